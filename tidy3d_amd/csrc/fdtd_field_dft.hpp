// Running DFT of a FieldMonitor on the nodes it keeps only (FDTD_MON_DFT_SPARSE; ref tidy3d monitor.py FieldMonitor with
// interval_space / colocate, base_sim/monitor.py:58-85).
//
// Colocation and the choice of every k-th node are linear, so the DFT of the colocated value is the colocated DFT: the accumulators
// exist on the kept nodes alone, and at every recorded step the sample is colocated from the fields at the moment
// dft_record_multi_kernel would have read them —
//     v = sum over the 2 x 2 x 2 taps of wx wy wz src[jz][jy][jx]          (colocate_taps of fdtd_field_time.hpp: the host's tap
//                                                                          tables, fp32, x then y then z of the caller's axes,
//                                                                          a tap of weight 0 not read)
//     acc[k][node] += v * phase[k]                                         (the expression of dft_record_multi_kernel)
// `src` is a box of one component, given by the address of its first sample and its row and plane strides (unit stride along x):
// the live field array at the box origin (strides g.nx, g.sxy), or the two-step sweep's copy of the middle step over the box
// (contiguous: strides bx, bx * by).  E components are recorded at the "pre" point with phase_e, H components at the "post" point
// with phase_h, as the whole-box DFT monitor's are; every schedule treats the monitor as the DFT monitor of its padded box.
//
// One thread per kept node, x fastest: a wave of 64 lanes owns (a piece of) one row of nodes, so its y and z taps are the same in
// every lane and its accumulator traffic is one contiguous run per frequency.  No atomics, no LDS: a node belongs to one thread,
// and the launches of one monitor follow one another on the stream that owns the fields.
#pragma once
#include <hip/hip_runtime.h>
#include "fdtd_field_time.hpp"

namespace fdtd {

struct FieldDftP {
  float2* acc;               // [nf][nodes]: per frequency the components one after the other, each [n2][n1][n0]
  const int* idx;            // taps: for component slot c and axis a, [nt[c][a]][2] indices into the box along a at off[c][a]
  const float* w;            //       their weights, same layout
  int off[6][3];
  int nt[6][3];              // kept nodes per component slot and axis
  long long out_off[6];      // where component slot c starts inside a frequency of `acc`
  long long nodes;           // kept nodes of all components
  int nf;
};
struct FieldDftSrc {         // the entries of one launch: component slots of the monitor and the box each is read from
  int n;
  int slot[6];
  const float* f[6];         // first sample of the box
  long long sy, sz;          // row and plane stride of the boxes
};

// blockIdx.x = piece of 64 nodes along x, blockIdx.y (strided) = group of kFieldTimeRows rows, blockIdx.z = entry of the launch.
// S: as field_time_gather_kernel (FDTD_OPT_AXIS_SHIFT).
template <int S>
__global__ __launch_bounds__(64 * kFieldTimeRows) void field_dft_record_kernel(FieldDftP p, FieldDftSrc r, const float2* phase) {
  const int e = (int)blockIdx.z;
  if (e >= r.n) return;
  const int c = r.slot[e];
  const int n0 = p.nt[c][0], n1 = p.nt[c][1], n2 = p.nt[c][2];
  const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (x >= n0) return;                                         // (no barrier below)
  const float* f = r.f[e];
  float2* a0 = p.acc + p.out_off[c];
  int j[3][2];
  float w[3][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { j[0][t] = p.idx[p.off[c][0] + 2 * x + t]; w[0][t] = p.w[p.off[c][0] + 2 * x + t]; }
  const long long rows = (long long)n1 * n2;
  for (long long row = (long long)blockIdx.y * kFieldTimeRows + threadIdx.y; row < rows; row += (long long)gridDim.y * kFieldTimeRows) {
    const int q1 = (int)(row % n1), q2 = (int)(row / n1);      // (the same in all 64 lanes of the wave)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      j[1][t] = p.idx[p.off[c][1] + 2 * q1 + t]; w[1][t] = p.w[p.off[c][1] + 2 * q1 + t];
      j[2][t] = p.idx[p.off[c][2] + 2 * q2 + t]; w[2][t] = p.w[p.off[c][2] + 2 * q2 + t];
    }
    const float v = colocate_taps<S>(f, r.sy, r.sz, j, w);
    const long long t = row * n0 + x;
    for (int k = 0; k < p.nf; ++k) {
      const float2 ph = phase[k];
      float2 a = a0[(long long)k * p.nodes + t];
      a.x += v * ph.x;
      a.y += v * ph.y;
      a0[(long long)k * p.nodes + t] = a;
    }
  }
}

}  // namespace fdtd
