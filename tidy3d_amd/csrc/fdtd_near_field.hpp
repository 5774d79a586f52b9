// K9b  exact projection (far_field_approx=False): the surface integrals of the homogeneous-medium Green's function without the
// far-field approximation (ref components/field_projection.py:831-1010; the host form is projection._exact_fields), sibling of K9
// (far_field_kernel).  One call = one surface of a projection monitor at one frequency.  In the surface's local frame (u, v, w =
// normal; the cross products below take it as right-handed, the host flips their sign for the one surface axis where it is not)
// with Rv = p - r', R = |Rv|, Rh = Rv / R and k = k_re + i k_im:
//
//     G  = exp(i k R) / (4 pi R),      G1 = G (i k - 1/R),      G2 = G1 (i k - 1/R) + G / R^2
//
// and for each current type F in {J, M} (tangential: F_w = 0), rd = Rh_u F_u + Rh_v F_v, twelve complex sums per point:
//
//     I_F[a] = sum w_u w_v [ G F_a + ( Rh_a rd G2 + (F_a - Rh_a rd) G1 / R ) / k^2 ]  =  sum w_u w_v [ A F_a + B Rh_a rd ]
//              A = G + G1 / (R k^2),   B = (G2 - G1 / R) / k^2                                     a in (u, v, w)
//     C_F[a] = sum w_u w_v G1 (Rh x F)_a
//
// out[n_pts][12][2] in the order I_J, I_M, C_J, C_M.  The host forms E = i w mu0 I_J - C_M, H = i w eps0 eps I_M + C_J: no physical
// constant enters here.  All arithmetic is fp64 (k R reaches 2e4 rad), sincos and exp from the math library, no fast-math form.
//
// Work split: one 256-thread workgroup per (point, lattice chunk); a thread takes the nodes q0 + t, q0 + t + 256, ... of its chunk in
// that order, the workgroup combines by the fixed LDS tree of K9 (three passes of eight values: 16 KiB), and where the lattice is cut
// into more than one chunk a second kernel adds the partial records in chunk order.  Nothing depends on the launch timing or on the
// device: the same inputs give the same bits on every run and every machine.  The chunk rule (near_field_chunks) is a function of
// n_pts and n_u * n_v alone:
//
//     wanted    = 64 below kNearPtsMany points, 8 below kNearPtsOne, 1 from there on
//     chunk_len = ceil(n / wanted) rounded up to a multiple of kNearChunkNodes,      chunks = ceil(n / chunk_len)  <=  wanted
//
// so few points still give up to 64 workgroups each, 128 points and more give at least 1024 workgroups whenever the lattice has the nodes
// for it, and no chunk is empty or shorter than 4 nodes per thread except the last.  The partial buffer holds n_pts * chunks records
// of 24 doubles, and only where chunks > 1:  n_pts * chunks <= max(127 * 64, 1023 * 8) = 8184 records < 1.5 MiB.
// A point that coincides with a lattice node has R = 0 and gives non-finite sums, as on the host; nothing treats it specially.
#pragma once
#include <hip/hip_runtime.h>

namespace fdtd {

constexpr int kNearChunkNodes = 1024;     // chunk lengths are multiples of this (4 nodes per thread)
constexpr int kNearPtsMany = 128;         // fewer points: up to 64 chunks
constexpr int kNearPtsOne = 1024;         // fewer points: up to 8 chunks; from here on the whole lattice in one workgroup

struct NearChunks { int chunks; long long chunk_len; };

inline NearChunks near_field_chunks(long long n_pts, long long n) {
  const long long wanted = n_pts < kNearPtsMany ? 64 : (n_pts < kNearPtsOne ? 8 : 1);
  const long long per = (n + wanted - 1) / wanted;
  NearChunks c;
  c.chunk_len = (per + kNearChunkNodes - 1) / kNearChunkNodes * kNearChunkNodes;
  c.chunks = (int)((n + c.chunk_len - 1) / c.chunk_len);
  return c;
}

struct NearP {
  const double* u; const double* v; const double* wu; const double* wv;
  const double2* cur;                    // [4][n_u * n_v]: J_u, J_v, M_u, M_v on the (u, v) lattice, v fastest
  int n_u, n_v;
  double w0, k_re, k_im;
  const double* p_u; const double* p_v; const double* p_w;      // observation points in the surface's (u, v, normal) frame
  int chunks; long long chunk_len;
  double* dst;                           // [n_pts][chunks][24]: the output itself where chunks == 1
};

__global__ __launch_bounds__(256) void near_field_kernel(NearP p) {
  __shared__ double red[256][8];
  const long long pt = (long long)blockIdx.x / p.chunks;
  const int chunk = (int)((long long)blockIdx.x - pt * p.chunks);
  const double pu = p.p_u[pt], pv = p.p_v[pt], dw = p.p_w[pt] - p.w0;
  const long long n = (long long)p.n_u * p.n_v;
  const long long q0 = (long long)chunk * p.chunk_len;
  const long long q1 = q0 + p.chunk_len < n ? q0 + p.chunk_len : n;
  // 1 / k^2
  const double k2r = p.k_re * p.k_re - p.k_im * p.k_im, k2i = 2.0 * p.k_re * p.k_im;
  const double k2n = 1.0 / (k2r * k2r + k2i * k2i);
  const double ikr = k2r * k2n, iki = -k2i * k2n;
  const double inv4pi = 0.25 / 3.14159265358979323846;
  double acc[24];
#pragma unroll
  for (int m = 0; m < 24; ++m) acc[m] = 0.0;
  for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
    const int iu = (int)(q / p.n_v), iv = (int)(q - (long long)iu * p.n_v);
    const double du = pu - p.u[iu], dv = pv - p.v[iv];
    const double R = sqrt(du * du + dv * dv + dw * dw);
    const double iR = 1.0 / R;
    const double hu = du * iR, hv = dv * iR, hw = dw * iR;
    double sn, cs;
    sincos(p.k_re * R, &sn, &cs);
    const double amp = (p.k_im != 0.0 ? exp(-p.k_im * R) : 1.0) * (inv4pi * iR) * (p.wu[iu] * p.wv[iv]);
    const double gr = amp * cs, gi = amp * sn;                        // w_u w_v G
    const double sr = -p.k_im - iR, si = p.k_re;                      // i k - 1/R
    const double g1r = gr * sr - gi * si, g1i = gr * si + gi * sr;    // w_u w_v G1
    const double g2r = g1r * sr - g1i * si + gr * iR * iR;            // w_u w_v G2
    const double g2i = g1r * si + g1i * sr + gi * iR * iR;
    const double tr = g1r * iR, ti = g1i * iR;                        // G1 / R
    const double ar = gr + (tr * ikr - ti * iki), ai = gi + (tr * iki + ti * ikr);
    const double dr = g2r - tr, di = g2i - ti;
    const double br = dr * ikr - di * iki, bi = dr * iki + di * ikr;
#pragma unroll
    for (int f = 0; f < 2; ++f) {                                     // J, M
      const double2 fu = p.cur[(long long)(2 * f) * n + q], fv = p.cur[(long long)(2 * f + 1) * n + q];
      const double rdr = hu * fu.x + hv * fv.x, rdi = hu * fu.y + hv * fv.y;
      const double er = br * rdr - bi * rdi, ei = br * rdi + bi * rdr;          // B rd
      acc[6 * f + 0] += (ar * fu.x - ai * fu.y) + hu * er;
      acc[6 * f + 1] += (ar * fu.y + ai * fu.x) + hu * ei;
      acc[6 * f + 2] += (ar * fv.x - ai * fv.y) + hv * er;
      acc[6 * f + 3] += (ar * fv.y + ai * fv.x) + hv * ei;
      acc[6 * f + 4] += hw * er;
      acc[6 * f + 5] += hw * ei;
      // Rh x F with F_w = 0:  (-Rh_w F_v,  Rh_w F_u,  Rh_u F_v - Rh_v F_u)
      const double xur = -hw * fv.x, xui = -hw * fv.y, xvr = hw * fu.x, xvi = hw * fu.y;
      const double xwr = hu * fv.x - hv * fu.x, xwi = hu * fv.y - hv * fu.y;
      acc[12 + 6 * f + 0] += g1r * xur - g1i * xui;
      acc[12 + 6 * f + 1] += g1r * xui + g1i * xur;
      acc[12 + 6 * f + 2] += g1r * xvr - g1i * xvi;
      acc[12 + 6 * f + 3] += g1r * xvi + g1i * xvr;
      acc[12 + 6 * f + 4] += g1r * xwr - g1i * xwi;
      acc[12 + 6 * f + 5] += g1r * xwi + g1i * xwr;
    }
  }
  double* dst = p.dst + (long long)blockIdx.x * 24;
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
    for (int m = 0; m < 8; ++m) red[threadIdx.x][m] = acc[8 * pass + m];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
#pragma unroll
        for (int m = 0; m < 8; ++m) red[threadIdx.x][m] += red[threadIdx.x + s][m];
      }
      __syncthreads();
    }
    if (threadIdx.x < 8) dst[8 * pass + threadIdx.x] = red[0][threadIdx.x];
    __syncthreads();
  }
}

// out[pt][j] = part[pt][0][j] + part[pt][1][j] + ... in chunk order; one thread per value
__global__ __launch_bounds__(256) void near_field_sum_kernel(const double* __restrict__ part, double* __restrict__ out, int chunks,
                                                             long long n_vals) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_vals) return;
  const long long pt = t / 24;
  const int j = (int)(t - pt * 24);
  const double* src = part + pt * chunks * 24 + j;
  double s = src[0];
  for (int c = 1; c < chunks; ++c) s += src[(long long)c * 24];
  out[t] = s;
}

}  // namespace fdtd
