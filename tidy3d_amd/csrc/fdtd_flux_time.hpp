// Flux through a planar surface at every recorded step, reduced on the device (FDTD_MON_FLUX_TIME; ref tidy3d monitor.py
// FluxTimeMonitor, monitor_data.py:1158 time-domain Poynting flux).
//
// Such a monitor records like a time monitor over its padded index box — the two tangential E and the two tangential H components,
// H already averaged to t_n — but into a ring of R records instead of one slot per recorded step (slot = record index mod R).  When
// the ring is full, at the end of a run and before the series is read, flux_time_reduce_kernel turns every complete record into one
// value:
//     flux[rec] = sign * sum over primal nodes (E_t1 H_t2 - E_t2 H_t1) * wi_x[i] * wi_y[j] * wi_z[k],     t1, t2 = axis + 1, axis + 2 (cyclic)
// each component colocated to the node first by the host's separable linear interpolation: per axis and component at most two
// taps (index into the box, weight) per node index — the same numbers data.py interpolates with.  A tap of weight 0 is not read.
//
// Fixed summation order, no atomics: a workgroup of 256 threads owns kFluxTile consecutive nodes of one record; thread t adds its
// nodes tile * kFluxTile + t, + 256, ... in that order, the 64 lanes of a wave combine by __shfl_down, the four waves through LDS,
// and the workgroup leaves ONE partial sum in partial[slot][tile].  flux_time_final_kernel adds the partials of a record in tile
// order.  So the value of a record depends on its contents alone — not on the schedule that wrote it, nor on how many records a
// launch covers.  fp32 throughout.
#pragma once
#include <hip/hip_runtime.h>

namespace fdtd {

constexpr int kFluxTile = 1024;       // nodes per workgroup (four per thread)
constexpr int kFluxMaxJobs = 8;       // monitors per launch
constexpr int kFluxMaxRing = 16384;   // records per ring at most (one grid row of the reduce launch per record)

struct FluxMonP {
  const float* stage;        // [ring][4][bz][by][bx]: E_t1, E_t2, H_t1, H_t2
  float* partial;            // [ring][tiles]
  float* result;             // [n_rec]
  const int* idx[3];         // per axis: [4][nt][2] tap indices into the box along that axis
  const float* w[3];         //           [4][nt][2] their weights
  const float* wi[3];        // per axis: [nt] integration weights (1 along the normal)
  int nt[3];                 // nodes per axis (1 along the normal)
  int b[3];                  // box extents bx, by, bz
  int tiles, ring;
  long long r0;              // records [r0, r0 + cnt) of this launch
  int cnt;
  float sign;
};
struct FluxLaunchP {
  int n;
  FluxMonP m[kFluxMaxJobs];
};

// blockIdx.x = tile, blockIdx.y = record of the launch, blockIdx.z = monitor of the launch
__global__ __launch_bounds__(256) void flux_time_reduce_kernel(FluxLaunchP L) {
  __shared__ float part[4];
  const FluxMonP& p = L.m[blockIdx.z];
  if ((int)blockIdx.x >= p.tiles || (int)blockIdx.y >= p.cnt) return;      // (the whole workgroup: a launch is as wide as its widest monitor)
  const int slot = (int)((p.r0 + blockIdx.y) % p.ring);
  const int bx = p.b[0], by = p.b[1];
  const long long cells = (long long)bx * by * p.b[2];
  const float* raw = p.stage + (long long)slot * 4 * cells;
  const int n0 = p.nt[0], n1 = p.nt[1], n2 = p.nt[2];
  const long long nodes = (long long)n0 * n1 * n2;
  float acc = 0.0f;
  for (int s = 0; s < kFluxTile / 256; ++s) {
    const long long t = (long long)blockIdx.x * kFluxTile + s * 256 + threadIdx.x;
    if (t >= nodes) continue;
    const int q0 = (int)(t % n0), q1 = (int)((t / n0) % n1), q2 = (int)(t / ((long long)n0 * n1));
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* f = raw + (long long)c * cells;
      const int* ix = p.idx[0] + ((long long)c * n0 + q0) * 2;
      const int* iy = p.idx[1] + ((long long)c * n1 + q1) * 2;
      const int* iz = p.idx[2] + ((long long)c * n2 + q2) * 2;
      const float* wx = p.w[0] + ((long long)c * n0 + q0) * 2;
      const float* wy = p.w[1] + ((long long)c * n1 + q1) * 2;
      const float* wz = p.w[2] + ((long long)c * n2 + q2) * 2;
      // x first, then y, then z: the order of the host's interpolation passes
      float sz = 0.0f;
      for (int cz = 0; cz < 2; ++cz) {
        if (wz[cz] == 0.0f) continue;
        float sy = 0.0f;
        for (int cy = 0; cy < 2; ++cy) {
          if (wy[cy] == 0.0f) continue;
          const float* row = f + ((long long)iz[cz] * by + iy[cy]) * bx;
          float sx = 0.0f;
          for (int cx = 0; cx < 2; ++cx)
            if (wx[cx] != 0.0f) sx = sx + wx[cx] * row[ix[cx]];
          sy = sy + wy[cy] * sx;
        }
        sz = sz + wz[cz] * sy;
      }
      v[c] = sz;
    }
    const float sn = v[0] * v[3] - v[1] * v[2];
    acc = acc + p.sign * sn * (p.wi[0][q0] * p.wi[1][q1] * p.wi[2][q2]);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[(long long)slot * p.tiles + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one thread per record of the launch: its partials in tile order.  blockIdx.y = monitor of the launch
__global__ __launch_bounds__(256) void flux_time_final_kernel(FluxLaunchP L) {
  const FluxMonP& p = L.m[blockIdx.y];
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.cnt) return;
  const long long rec = p.r0 + q;
  const float* part = p.partial + (rec % p.ring) * p.tiles;
  float s = 0.0f;
  for (int t = 0; t < p.tiles; ++t) s = s + part[t];
  p.result[rec] = s;
}

}  // namespace fdtd
