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
  float2* acc;               // [nf][t.nodes]: per frequency the components one after the other, each [n2][n1][n0]
  TapTables t;
  int nf;
};
struct FieldDftSrc {         // the entries of one launch: component slots of the monitor and the box each is read from
  int n;
  int slot[6];
  const float* f[6];         // first sample of the box
  long long sy, sz;          // row and plane stride of the boxes
};

// blockIdx.z = entry of the launch; x, y and S: for_each_kept_node (fdtd_field_time.hpp).
template <int S>
__global__ __launch_bounds__(64 * kFieldTimeRows) void field_dft_record_kernel(FieldDftP p, FieldDftSrc r, const float2* phase) {
  const int e = (int)blockIdx.z;
  if (e >= r.n) return;
  const int c = r.slot[e];
  const int x = kept_x();
  if (x >= p.t.nt[c][0]) return;                               // (no barrier below)
  float2* a0 = p.acc + p.t.out_off[c];
  for_each_kept_node<S>(p.t, c, x, r.f[e], r.sy, r.sz, [&](long long node, float v) {
    for (int k = 0; k < p.nf; ++k) {
      const float2 ph = phase[k];
      float2 a = a0[(long long)k * p.t.nodes + node];
      a.x += v * ph.x;
      a.y += v * ph.y;
      a0[(long long)k * p.t.nodes + node] = a;
    }
  });
}

}  // namespace fdtd
