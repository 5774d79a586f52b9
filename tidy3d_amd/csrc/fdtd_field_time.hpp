// Field values on the nodes a FieldTimeMonitor keeps, gathered on the device (FDTD_MON_TIME_SPARSE; ref tidy3d monitor.py
// FieldTimeMonitor with interval_space / colocate, base_sim/monitor.py:58-85).
//
// Such a monitor records like a time monitor over its padded index box — every component, H already averaged to t_n — but into a
// ring of R records instead of one slot per recorded step (slot = record index mod R; the ring bookkeeping is the flux-time
// monitor's, fdtd_capi.hip ring_drain).  When the ring is full, at the end of a run and before the result is read,
// field_time_gather_kernel turns every complete record into the values on the kept nodes:
//     out[rec][comp][kz][ky][kx] = sum over the 2 x 2 x 2 taps of wx wy wz raw[slot][comp][jz][jy][jx]
// by the host's separable linear interpolation: per axis, component and node two taps (index into the box, weight) — the same
// numbers data.py interpolates with (colocation to the primal nodes and / or the choice of every k-th node), applied in the
// host's order: x, then y, then z of the caller's axes.  A tap of weight 0 is not read: whatever lies under it, a NaN included, stays out.  fp32.
//
// One thread per kept node, x fastest: a wave of 64 lanes owns (a piece of) one row of nodes, so its y and z taps are the same in
// every lane and its stores are one contiguous run.  No atomics, no LDS; a value depends on the contents of its record alone.
#pragma once
#include <hip/hip_runtime.h>

namespace fdtd {

constexpr int kFieldTimeRows = 4;       // rows of nodes (waves) per workgroup
constexpr int kFieldTimeMaxRowBlocks = 16384;     // grid rows of a launch at most (a workgroup strides the rest)

// The tap tables of a sparse monitor, shared by FieldTimeP and FieldDftP (fdtd_field_dft.hpp): filled and uploaded by tap_tables
// (fdtd_capi.hip), walked by for_each_kept_node.
struct TapTables {
  const int* idx;            // taps: for component slot c and axis a, [nt[c][a]][2] indices into the box along a at off[c][a]
  const float* w;            //       their weights, same layout
  int off[6][3];
  int nt[6][3];              // kept nodes per component slot and axis
  long long out_off[6];      // where component slot c starts inside a record / a frequency of the result
  long long nodes;           // kept nodes of all components
};
struct FieldTimeP {
  const float* stage;        // [ring][n_comps][bz][by][bx]
  float* out;                // [n_rec][t.nodes]: per record the components one after the other, each [n2][n1][n0]
  TapTables t;
  int b[3];                  // box extents bx, by, bz
  int n_comps, ring;
  long long r0;              // records [r0, r0 + cnt) of this launch
  int cnt;
};

// The value on one kept node: sum over the 2 x 2 x 2 taps of wx wy wz f[jz * sz + jy * sy + jx] — `f` a box of one component with
// unit stride along x — formed separably along the caller's x, then y, then z (S as below), fp32; what lies under a zero weight is
// not read.  Shared with field_dft_record_kernel (fdtd_field_dft.hpp): one set of operations for both.
template <int S>
__device__ __forceinline__ float colocate_taps(const float* f, long long sy, long long sz, const int (&j)[3][2], const float (&w)[3][2]) {
  constexpr int A0 = (3 - S) % 3, A1 = (4 - S) % 3, A2 = (5 - S) % 3;
  float v[2][2][2];                                            // [z tap][y tap][x tap]
#pragma unroll
  for (int cz = 0; cz < 2; ++cz)
#pragma unroll
    for (int cy = 0; cy < 2; ++cy)
#pragma unroll
      for (int cx = 0; cx < 2; ++cx)
        v[cz][cy][cx] = (w[2][cz] != 0.0f && w[1][cy] != 0.0f && w[0][cx] != 0.0f) ? f[(long long)j[2][cz] * sz + (long long)j[1][cy] * sy + j[0][cx]] : 0.0f;
  float t1[2][2], t2[2];                                       // after the first pass [tap along A2][tap along A1], after the second [tap along A2]
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) {
#pragma unroll
    for (int c1 = 0; c1 < 2; ++c1) {
      float s = 0.0f;
#pragma unroll
      for (int c0 = 0; c0 < 2; ++c0) {
        int t[3];
        t[A0] = c0; t[A1] = c1; t[A2] = c2;
        if (w[A0][c0] != 0.0f) s = s + w[A0][c0] * v[t[2]][t[1]][t[0]];
      }
      t1[c2][c1] = s;
    }
    float s = 0.0f;
#pragma unroll
    for (int c1 = 0; c1 < 2; ++c1)
      if (w[A1][c1] != 0.0f) s = s + w[A1][c1] * t1[c2][c1];
    t2[c2] = s;
  }
  float s = 0.0f;
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
    if (w[A2][c2] != 0.0f) s = s + w[A2][c2] * t2[c2];
  return s;
}

// The kept nodes of component slot `c` that belong to this thread — node `x` (< nt[c][0]: a thread beyond has returned, kept_x)
// of the rows blockIdx.y (strided) = group of kFieldTimeRows rows: sink(index of the node inside the component, its value
// colocated from the box `f`) for each.
// S = the cyclic renaming the caller laid the problem out with (FDTD_OPT_AXIS_SHIFT: device axis a holds the caller's axis (a + S) % 3):
// the three passes run along the caller's x, y, z — device axes (3 - S) % 3, (4 - S) % 3, (5 - S) % 3 — so that a renamed problem
// gives the bits of the plain one.
__device__ __forceinline__ int kept_x() { return (int)blockIdx.x * 64 + (int)threadIdx.x; }      // blockIdx.x = piece of 64 nodes along x
template <int S, class Sink>
__device__ __forceinline__ void for_each_kept_node(const TapTables& T, int c, int x, const float* f, long long sy, long long sz, Sink&& sink) {
  const int n0 = T.nt[c][0], n1 = T.nt[c][1], n2 = T.nt[c][2];
  int j[3][2];
  float w[3][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { j[0][t] = T.idx[T.off[c][0] + 2 * x + t]; w[0][t] = T.w[T.off[c][0] + 2 * x + t]; }
  const long long rows = (long long)n1 * n2;
  for (long long row = (long long)blockIdx.y * kFieldTimeRows + threadIdx.y; row < rows; row += (long long)gridDim.y * kFieldTimeRows) {
    const int q1 = (int)(row % n1), q2 = (int)(row / n1);      // (the same in all 64 lanes of the wave)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      j[1][t] = T.idx[T.off[c][1] + 2 * q1 + t]; w[1][t] = T.w[T.off[c][1] + 2 * q1 + t];
      j[2][t] = T.idx[T.off[c][2] + 2 * q2 + t]; w[2][t] = T.w[T.off[c][2] + 2 * q2 + t];
    }
    sink(row * n0 + x, colocate_taps<S>(f, sy, sz, j, w));
  }
}

// blockIdx.z = record of the launch x component; x, y and S: for_each_kept_node.
template <int S>
__global__ __launch_bounds__(64 * kFieldTimeRows) void field_time_gather_kernel(FieldTimeP p) {
  const int c = (int)(blockIdx.z % (unsigned)p.n_comps), q = (int)(blockIdx.z / (unsigned)p.n_comps);
  if (q >= p.cnt) return;
  const int x = kept_x();
  if (x >= p.t.nt[c][0]) return;                               // (no barrier below)
  const long long rec = p.r0 + q;
  const int slot = (int)(rec % p.ring);
  const int bx = p.b[0], by = p.b[1];
  const long long cells = (long long)bx * by * p.b[2];
  float* o = p.out + rec * p.t.nodes + p.t.out_off[c];
  for_each_kept_node<S>(p.t, c, x, p.stage + ((long long)slot * p.n_comps + c) * cells, (long long)bx, (long long)bx * by,
                        [&](long long node, float v) { o[node] = v; });
}

}  // namespace fdtd
