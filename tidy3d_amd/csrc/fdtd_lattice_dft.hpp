// Running DFT of a projection monitor's surface on its sampling lattice only (FDTD_MON_DFT_LATTICE; ref tidy3d monitor.py
// FieldProjectionAngleMonitor / ...CartesianMonitor / ...KSpaceMonitor, field_projection.py:280-349: the equivalent currents are
// sampled on a regular lattice of 10 points per wavelength).
//
// The host path holds the four tangential components over every cell of the padded surface box, colocates them to the primal
// nodes after the run and resamples those to the lattice.  Both steps are linear, so — the argument of fdtd_field_dft.hpp — the
// accumulators can live on the lattice alone.  A lattice point lies between two colocated nodes, each of which has two Yee taps:
// four taps per axis (data.lattice_taps: node j tap 0, node j tap 1, node j + 1 tap 0, node j + 1 tap 1, each weight the product
// of the lattice weight and the colocation weight, formed in float64 and cast once), where the sparse form of
// fdtd_field_time.hpp carries two.  At every recorded step, from the fields at the moment dft_record_multi_kernel would have
// read them —
//     v = sum over the 4 x 4 x 4 slots of wx wy wz src[jz][jy][jx]          (separable: along the caller's x, then y, then z; fp32;
//                                                                          the slots in table order; a slot of weight 0 is
//                                                                          neither read nor added)
//     acc[k][node] += v * phase[k]                                         (the expression of dft_record_multi_kernel)
// `src`, the phase row and the schedules: FieldDftSrc, fdtd_field_dft.hpp.  The tables are TapTables with kLatticeTaps entries per
// node and axis instead of two.
//
// Lanes.  These are planes: along its normal a surface keeps one node.  for_each_kept_node lays the 64 lanes of a wave along x,
// which on a surface normal to x (nt[c][0] == 1) would run one lane in 64.  Here the lanes lie along the first axis L on which the
// component keeps more than one node, and a wave's rows are counted over the axes behind it; the axes in front of L keep one node.
// The result stays [n2][n1][n0], so with p the lane's node along L and `row` the wave's row
//     normal z (n2 == 1):  L = 0, row = q1         node = q1 * n0 + p      = row * n0 + p
//     normal y (n1 == 1):  L = 0, row = q2         node = q2 * n0 + p      = row * n0 + p
//     normal x (n0 == 1):  L = 1, row = q2         node = q2 * n1 + p      = row * n1 + p
//     (a line along z, n0 == n1 == 1: L = 2, one row, node = p)
// in every orientation node = row * nt[L] + p: the 64 lanes of a wave read and write 64 consecutive float2 of each frequency — one
// contiguous run of 512 B per frequency, as in the volume kernel.  (The field reads of a surface normal to x are strided by the
// row length whatever the mapping: its samples lie one per row of the grid.)
//
// Registers.  Up to 4 x 4 x 2 = 32 samples per node carry weight (the normal axis has two slots of weight 0).  They are not
// gathered into an array first: the three nested sums run as one stream, each sample multiplied into the running sum of its x
// pass as it arrives, so a thread holds its 24 taps (those of the two row axes are the same in every lane: the row is made
// wave-uniform with readfirstlane, they are scalar loads), three partial sums and the samples in flight.  The lane axis is a
// template parameter, so no register array is indexed at run time: no scratch (scripts/kernel_resources.py).
// No atomics, no LDS: a node belongs to one thread, and the launches of one monitor follow one another on the stream that owns
// the fields.
#pragma once
#include <hip/hip_runtime.h>
#include "fdtd_field_dft.hpp"

namespace fdtd {

constexpr int kLatticeTaps = 4;         // slots per node and axis

// The lane axis of component slot c: the first axis on which it keeps more than one node (2 if it keeps a single node).
__host__ __device__ inline int lattice_lane_axis(const TapTables& T, int c) { return T.nt[c][0] > 1 ? 0 : T.nt[c][1] > 1 ? 1 : 2; }
// ... and its rows: the nodes over the axes behind the lane axis
__host__ __device__ inline long long lattice_rows(const TapTables& T, int c, int L) {
  return L == 0 ? (long long)T.nt[c][1] * T.nt[c][2] : L == 1 ? (long long)T.nt[c][2] : 1;
}

// The value on one lattice node: the separable 4-tap sums along the caller's x, then y, then z (S: for_each_kept_node) of the box
// `f` (unit stride along x), the slots in table order, fp32; what lies under a zero weight is neither read nor added.
template <int S>
__device__ __forceinline__ float lattice_value(const float* f, long long sy, long long sz, const int (&j)[3][kLatticeTaps],
                                               const float (&w)[3][kLatticeTaps]) {
  constexpr int A0 = (3 - S) % 3, A1 = (4 - S) % 3, A2 = (5 - S) % 3;
  float s2 = 0.0f;
#pragma unroll
  for (int c2 = 0; c2 < kLatticeTaps; ++c2) {
    if (w[A2][c2] == 0.0f) continue;
    float s1 = 0.0f;
#pragma unroll
    for (int c1 = 0; c1 < kLatticeTaps; ++c1) {
      if (w[A1][c1] == 0.0f) continue;
      float s0 = 0.0f;
#pragma unroll
      for (int c0 = 0; c0 < kLatticeTaps; ++c0) {
        if (w[A0][c0] == 0.0f) continue;
        int t[3];
        t[A0] = c0; t[A1] = c1; t[A2] = c2;
        s0 = s0 + w[A0][c0] * f[(long long)j[2][t[2]] * sz + (long long)j[1][t[1]] * sy + j[0][t[0]]];
      }
      s1 = s1 + w[A1][c1] * s0;
    }
    s2 = s2 + w[A2][c2] * s1;
  }
  return s2;
}

// The nodes of component slot `c` that belong to this thread, the lanes along axis L (< 3: the component's lattice_lane_axis):
// node p = blockIdx.x * 64 + threadIdx.x along L of the rows blockIdx.y (strided) = group of kFieldTimeRows rows.
template <int S, int L>
__device__ __forceinline__ void lattice_record(const FieldDftP& P, int c, const float* f, long long sy, long long sz, const float2* phase) {
  const TapTables& T = P.t;
  const int nl = T.nt[c][L];
  const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (p >= nl) return;                                         // (no barrier below)
  int j[3][kLatticeTaps];
  float w[3][kLatticeTaps];
  auto taps = [&](int a, int q) {
#pragma unroll
    for (int t = 0; t < kLatticeTaps; ++t) { j[a][t] = T.idx[T.off[c][a] + kLatticeTaps * q + t]; w[a][t] = T.w[T.off[c][a] + kLatticeTaps * q + t]; }
  };
  taps(L, p);
  if constexpr (L >= 1) taps(0, 0);                                      // the axes in front of the lane axis keep one node
  if constexpr (L == 2) taps(1, 0);
  const int n1 = T.nt[c][1];
  const long long rows = lattice_rows(T, c, L);
  const int wave_row = __builtin_amdgcn_readfirstlane((int)threadIdx.y);     // one row per wave: the row and its taps are wave-uniform
  float2* a0 = P.acc + T.out_off[c];
  for (long long row = (long long)blockIdx.y * kFieldTimeRows + wave_row; row < rows; row += (long long)gridDim.y * kFieldTimeRows) {
    if constexpr (L == 0) { taps(1, (int)(row % n1)); taps(2, (int)(row / n1)); }
    if constexpr (L == 1) taps(2, (int)row);
    const float v = lattice_value<S>(f, sy, sz, j, w);
    const long long node = row * nl + p;
    for (int k = 0; k < P.nf; ++k) {
      const float2 ph = phase[k];
      float2 a = a0[(long long)k * T.nodes + node];
      a.x += v * ph.x;
      a.y += v * ph.y;
      a0[(long long)k * T.nodes + node] = a;
    }
  }
}

// blockIdx.z = entry of the launch; x, y: lattice_record; S: for_each_kept_node (fdtd_field_time.hpp).
template <int S>
__global__ __launch_bounds__(64 * kFieldTimeRows) void lattice_dft_record_kernel(FieldDftP p, FieldDftSrc r, const float2* phase) {
  const int e = (int)blockIdx.z;
  if (e >= r.n) return;
  const int c = r.slot[e];
  switch (lattice_lane_axis(p.t, c)) {                         // (the same in every thread of the launch's entry)
    case 0: lattice_record<S, 0>(p, c, r.f[e], r.sy, r.sz, phase); break;
    case 1: lattice_record<S, 1>(p, c, r.f[e], r.sy, r.sz, phase); break;
    default: lattice_record<S, 2>(p, c, r.f[e], r.sy, r.sz, phase); break;
  }
}

}  // namespace fdtd
