// K12  staircase rasterisation of Box, Sphere and Cylinder structures (discretize.rasterize, the host path, is the reference: the
// result is held to it bit for bit).  One launch paints the node index box of ONE structure for ONE E component into that component's
// uint16 volume [nz][ny][nx]; the launches of a call go to one stream in the order of the structures, so a later structure overwrites
// an earlier one exactly as the host's assignments do.  No atomics, no LDS: a thread owns one x node of one (z, y) row, loads the
// node's three fp64 Yee coordinates, evaluates the primitive's ``inside`` test and stores the medium index where it passes.
//
// The tests restate schema.Box.inside / Sphere.inside / Cylinder.inside operation by operation (NumPy evaluates them in fp64 with
// one rounding per operation, ``a ** 2`` as a * a):
//
//     box       |x - x0| <= 0.5 Lx  &  |y - y0| <= 0.5 Ly  &  |z - z0| <= 0.5 Lz                    (0.5 L is exact; inf stays inf)
//     sphere    ((x - x0)^2 + (y - y0)^2) + (z - z0)^2 <= r2             r2 = ``radius ** 2`` as the host's Python evaluates it
//     cylinder  r > 0  &  (p0 - c0)^2 + (p1 - c1)^2 <= r * r  &  |pa - ca| <= 0.5 len       a = axis, (p0, p1) the other two in x, y, z
//                                                                                  order, len = min(length, 1e10)
//
// THIS TRANSLATION UNIT MUST BE BUILT WITH -ffp-contract=off (tidy3d_amd/build.py does so for every unit of the library): a
// difference and its square, or two squares and their sum, contracted into an FMA round once instead of twice and move nodes that
// lie on a surface (tests/raster_case.py holds scenes that tell the two builds apart).  No fast-math, no float.
//
// Launch shape: 64 x 4 threads — a wave is 64 consecutive x nodes of one row (128-byte stores), a workgroup four rows of one plane;
// grid = (ceil(bx / 64), ceil(by / 4), bz) over the index box.  The caller (fdtd_rasterize) checks the box against the shape and
// by, bz against the 65535 limit of grid.y / grid.z before any launch.
#pragma once
#include <hip/hip_runtime.h>

namespace fdtd {

constexpr int kRasterBox = 0, kRasterSphere = 1, kRasterCylinder = 2;
constexpr int kRasterLanes = 64, kRasterRows = 4;

struct RasterP {
  const double* xs; const double* ys; const double* zs;      // Yee coordinates of this component: nx, ny, nz values
  unsigned short* out;                                       // this component's volume [nz][ny][nx]
  int nx, ny;
  int lo0, lo1, lo2, hi0, hi1, hi2;                          // index box [lo, hi) along x, y, z
  double c0, c1, c2;                                         // centre
  double s0, s1, s2;                                         // box: size; sphere: r2, -, -; cylinder: radius, length (finite), -
  int axis;                                                  // cylinder
  unsigned short medium;
};

template <int SHAPE>
__device__ inline bool raster_inside(const RasterP& p, double x, double y, double z) {
  if (SHAPE == kRasterBox) {
    return fabs(x - p.c0) <= 0.5 * p.s0 && fabs(y - p.c1) <= 0.5 * p.s1 && fabs(z - p.c2) <= 0.5 * p.s2;
  } else if (SHAPE == kRasterSphere) {
    const double dx = x - p.c0, dy = y - p.c1, dz = z - p.c2;
    return (dx * dx + dy * dy) + dz * dz <= p.s0;
  } else {
    double p0, p1, pa, c0, c1, ca;
    if (p.axis == 0)      { pa = x; ca = p.c0; p0 = y; c0 = p.c1; p1 = z; c1 = p.c2; }
    else if (p.axis == 1) { pa = y; ca = p.c1; p0 = x; c0 = p.c0; p1 = z; c1 = p.c2; }
    else                  { pa = z; ca = p.c2; p0 = x; c0 = p.c0; p1 = y; c1 = p.c1; }
    const double d0 = p0 - c0, d1 = p1 - c1, r = p.s0;
    return r > 0.0 && d0 * d0 + d1 * d1 <= r * r && fabs(pa - ca) <= 0.5 * p.s1;
  }
}

template <int SHAPE>
__global__ __launch_bounds__(kRasterLanes * kRasterRows) void raster_paint_kernel(RasterP p) {
  const int i = p.lo0 + (int)blockIdx.x * kRasterLanes + (int)threadIdx.x;
  const int j = p.lo1 + (int)blockIdx.y * kRasterRows + (int)threadIdx.y;
  const int k = p.lo2 + (int)blockIdx.z;
  if (i >= p.hi0 || j >= p.hi1 || k >= p.hi2) return;
  if (raster_inside<SHAPE>(p, p.xs[i], p.ys[j], p.zs[k]))
    p.out[((long long)k * p.ny + j) * p.nx + i] = p.medium;
}

// the background: every entry of the three volumes = `value`; n16 stores of eight entries (the allocation is rounded up to them)
__global__ __launch_bounds__(256) void raster_fill_kernel(uint4* out, long long n16, unsigned value) {
  const unsigned w = value | (value << 16);
  uint4 v;
  v.x = w; v.y = w; v.z = w; v.w = w;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n16; q += (long long)gridDim.x * 256) out[q] = v;
}

}  // namespace fdtd
