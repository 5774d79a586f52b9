// Translation unit of the two-steps-per-sweep kernels (fdtd_kernels2.hpp) and their host-side launchers.
// Built with -fno-slp-vectorize (tidy3d_amd/build.py): see fdtd_fused2.hpp.
#include "fdtd_static_kernels.hpp"
#include "fdtd_kernels2.hpp"

namespace fdtd {

void launch_inject_values(hipStream_t st, float* val, const float* w_re, const float* w_im, const float2* wave,
                          long long step, int n) {
  hipLaunchKernelGGL(inject_values_kernel, dim3(1), dim3(256), 0, st, val, w_re, w_im, wave, step, n);
}

// its own instantiations: the whole grid, and the deferred-seam forms a run of plain pairs uses
static FDTD_F2_LAUNCHER(launch_fused2_step_base, FDTD_F2_LIST_OWN)

bool launch_fused2_step(const Fused2Launch& L) {
  if (L.opt & kF2Src) return launch_fused2_step_src(L);
  if (fused2_whatif(L.opt)) return launch_fused2_step_whatif(L);
  if (L.opt & kF2Disp) return launch_fused2_step_disp(L);
  if (L.opt & kF2Clip) return launch_fused2_step_clip(L);
  return launch_fused2_step_base(L);
}

void launch_inject_table(hipStream_t st, float* tab, long long stride, long long off, const float* w_re, const float* w_im,
                         const float2* wave, long long n_steps, int n) {
  const unsigned blocks = (unsigned)((n_steps * n + 255) / 256);
  hipLaunchKernelGGL(inject_table_kernel, dim3(blocks), dim3(256), 0, st, tab, stride, off, w_re, w_im, wave, n_steps, n);
}

void launch_pair_record(hipStream_t st, const PairRecP& r, long long max_cells, const GridP& g, const FieldP& a, const FieldP& b,
                        const float* cap) {
  const dim3 grid((unsigned)((max_cells + 255) / 256), (unsigned)(r.n_mon * 6));
  hipLaunchKernelGGL(pair_record_kernel, grid, dim3(256), 0, st, r, g, a, b, cap);
}

void launch_dft_record_dump(hipStream_t st, const DftDumpP& r, const float* dump, float2* acc, long long cells, long long fstride,
                            const float2* phase, int nf) {
  const dim3 grid((unsigned)((cells + 255) / 256), (unsigned)r.n);
  hipLaunchKernelGGL(dft_record_dump_kernel, grid, dim3(256), 0, st, r, dump, acc, cells, fstride, phase, nf);
}

void launch_seams(hipStream_t st, const GridP& g, const FieldP& b, const StepP& s, const MatP& m, const float* seam,
                  int n_seams, const DampT& dmp, const ClipP& clip, const InjP& inj, const SrcP& sr, float* rep) {
  const long long nt = (long long)n_seams * (clip.j1 - clip.j0) * (clip.k1 - clip.k0);
  if (nt <= 0) return;
  const unsigned blocks = (unsigned)((nt + 255) / 256);
  hipLaunchKernelGGL(seam_kernel, dim3(blocks), dim3(256), 0, st, g, b, s, m, seam, n_seams, dmp, clip, inj, sr, rep);
}

void launch_seam_flush(hipStream_t st, const GridP& g, const FieldP& b, const float* rep, int n_seams) {
  const long long nt = (long long)n_seams * g.ny * g.nz;
  if (nt <= 0) return;
  hipLaunchKernelGGL(seam_flush_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, g, b, rep, n_seams);
}

}  // namespace fdtd
