// One time step per sweep: the dispatch of fused_step_kernel<MAT, LB, PML, HINT, WIDE> (the kernel lives in fdtd_kernels.hpp; its
// instantiations are compiled in fdtd_capi.hip, where FDTD_F1_LAUNCHER stands in front of launch_fused_range).  Here: the word of a
// launch, the rules that form it, the one list of instantiations that exist, and the launcher's interface (the form of fdtd_fused2.hpp).
#pragma once
#include "fdtd_kernels.hpp"

namespace fdtd {

// ---- the word (MATF, LB, PML, HINT) of a launch ------------------------------------------------------------------------------------
// MATF: 0 = uniform medium <false, ., ., .>, 1 = packed medium words + LDS table <true, ., ., .>, 2 = the wide table
// <true, ., ., ., true>.  LB: the kernel's __launch_bounds__ (its register budget).  PML, HINT: the kernel's template arguments.
struct FusedWord { int matf, lb, pml, hint; };

// axes whose CPML recursions the launch carries -> the instantiation: none, the x-only one, the all-axes one (axes outside
// `pml_inside` have no members in the parameter block)
constexpr int fused_pml_form(int pml_inside) { return pml_inside == 0 ? 0 : (pml_inside == 1 ? 1 : 7); }

// The launch bound of a workgroup of `threads`: the one asked for (FDTD_OPT_FUSED_LB; 0 = by workgroup size: 256 / 512 / 1024 threads),
// never below the workgroup.  The CPML-carrying sweeps have two bounds: any bound other than 256 is their 512 form (a request of 1024
// on a CPML grid runs it).  The fold stands in front of the raise, so a bound never falls below `threads`: up to 512 threads the
// order makes no difference, and a CPML-carrying workgroup of more than 512 threads gets the bound 1024, which has no CPML form —
// launch_fused_step refuses it (callers keep such workgroups away: sweep_pml_axes, shell_why_not, pml_in_m in Run::setup).
constexpr int fused_lb(int threads, int requested, int pml_form) {
  int lb = requested ? requested : (threads <= 256 ? 256 : (threads <= 512 ? 512 : 1024));
  if (pml_form != 0 && lb != 256) lb = 512;
  if (lb < threads) lb = threads <= 512 ? 512 : 1024;
  return lb;
}

// Non-temporal field stores (FDTD_OPT_MEM_HINTS) in the instantiations WITHOUT CPML only: measured inside one engine
// (profiles/r02z_probe_same_engine_cache_hints.jsonl) they take 2.1 % off the plain sweep and 3.1 % off the one with
// materials, and ADD 13 % to the CPML-carrying ones (2-3 waves per SIMD: the slower store completion is not hidden).
// With them goes the order of the stores: H ahead of the row exchange instead of behind the E update (-0.5 % there,
// +12 % in the CPML-carrying instantiations; raising the wave priority while a plane's loads go out: +0.6 %;
// profiles/r03k_probe_early_h_stores_setprio.jsonl).
// The CPML-carrying instantiations store their H-side psi behind the E update instead of in the H phase in front of
// the row exchange: -2.7 ... -3.3 % of the whole CPML step (profiles/r04j_probe_late_psi_h_stores_all.jsonl).
// Non-temporal field stores on top of that: +13 % again (r04k).
// Without CPML (256-thread instantiations) the E values of a plane are stored one H phase later, behind the loads of
// the next plane (12 more live registers): -0.3 ... -0.9 % (r04l); the same in the CPML instantiations: +10 % (r04m).
constexpr int fused_hint(int lb, int pml_form, int mem_hints) {
  if (!mem_hints) return 0;
  if (pml_form != 0) return 128;
  return lb == 256 ? 265 : 9;
}

constexpr FusedWord fused_word(int matf, int threads, int requested, int pml_inside, int mem_hints) {
  const int pml = fused_pml_form(pml_inside), lb = fused_lb(threads, requested, pml);
  return FusedWord{matf, lb, pml, fused_hint(lb, pml, mem_hints)};
}

// dynamic LDS of a workgroup of `rows_plus_halo` waves: the double-buffered row exchange (H_x, H_z), and the x coefficients both CPML
// instantiations stage (the caller adds FDTD_OPT_LDS_PAD)
constexpr size_t fused_lds_bytes(int rows_plus_halo, int pml_form) {
  return ((size_t)2 * 2 * rows_plus_halo * 64 + (pml_form ? 6 * 64 : 0)) * sizeof(float4);
}

// ---- the instantiations that exist: one list of X(MATF, LB, PML, HINT) ---------------------------------------------------------------
// Without CPML three bounds, hinted 265 at 256 threads and 9 above; with CPML (x only / all axes) two bounds, hinted 128.  A word
// outside the list is refused, never mapped to a neighbour.
#define FDTD_F1_HINTED(X, M, LB, P, H) X(M, LB, P, 0) X(M, LB, P, H)
#define FDTD_F1_PLAIN(X, M) FDTD_F1_HINTED(X, M, 256, 0, 265) FDTD_F1_HINTED(X, M, 512, 0, 9) FDTD_F1_HINTED(X, M, 1024, 0, 9)
#define FDTD_F1_CPML(X, M, P) FDTD_F1_HINTED(X, M, 256, P, 128) FDTD_F1_HINTED(X, M, 512, P, 128)
#define FDTD_F1_MATF(X, M) FDTD_F1_PLAIN(X, M) FDTD_F1_CPML(X, M, 1) FDTD_F1_CPML(X, M, 7)
#define FDTD_F1_LIST(X) FDTD_F1_MATF(X, 0) FDTD_F1_MATF(X, 1) FDTD_F1_MATF(X, 2)
// the word as one switch value (a word listed twice is a duplicate case label)
constexpr int fused_key(int matf, int lb, int pml, int hint) { return ((matf * 2048 + lb) * 8 + pml) * 512 + hint; }
constexpr bool fused_instantiated(int matf, int lb, int pml, int hint) {
  switch (fused_key(matf, lb, pml, hint)) {
#define FDTD_F1_X(M, LBV, PV, HV) case fused_key(M, LBV, PV, HV):
    FDTD_F1_LIST(FDTD_F1_X)
#undef FDTD_F1_X
      return true;
    default: return false;
  }
}
constexpr bool fused_instantiated(const FusedWord& w) { return fused_instantiated(w.matf, w.lb, w.pml, w.hint); }
// every word launch_fused_range can form — 1 ... 15 rows per workgroup, every value FDTD_OPT_FUSED_LB takes, every set of in-sweep
// axes, with and without hints — has its instantiation, under a bound that holds its workgroup; a CPML-carrying workgroup of more
// than 512 threads has none: a new rule without its kernel stops the build, not a run
constexpr bool fused_words_instantiated() {
  const int lb_requests[4] = {0, 256, 512, 1024};
  for (int matf = 0; matf <= 2; ++matf)
    for (int threads = 128; threads <= 1024; threads += 64)
      for (int requested : lb_requests)
        for (int pml_inside = 0; pml_inside <= 7; ++pml_inside)
          for (int hints = 0; hints <= 1; ++hints) {
            const FusedWord w = fused_word(matf, threads, requested, pml_inside, hints);
            const bool refused = w.pml != 0 && threads > 512;
            if (fused_instantiated(w) == refused) return false;
            if (!refused && w.lb < threads) return false;
          }
  return true;
}
static_assert(fused_words_instantiated(), "fused_word forms a word that the list of instantiations does not hold (or holds one for a CPML-carrying workgroup of more than 512 threads)");
#define FDTD_F1_X(M, LBV, PV, HV) +1
static_assert(0 FDTD_F1_LIST(FDTD_F1_X) == 42, "fused_step_kernel: 14 instantiations per material form");
#undef FDTD_F1_X

// the rules pinned in bare numbers (independent of the names above)
constexpr bool fused_word_is(const FusedWord& w, int matf, int lb, int pml, int hint) { return w.matf == matf && w.lb == lb && w.pml == pml && w.hint == hint; }
static_assert(fused_word_is(fused_word(1, 320, 0, 0, 1), 1, 512, 0, 9) && fused_word_is(fused_word(0, 256, 0, 0, 1), 0, 256, 0, 265) &&
              fused_word_is(fused_word(2, 512, 0, 6, 1), 2, 512, 7, 128) && fused_word_is(fused_word(0, 192, 1024, 1, 0), 0, 512, 1, 0) &&
              fused_word_is(fused_word(1, 1024, 0, 0, 0), 1, 1024, 0, 0) && fused_word_is(fused_word(0, 192, 1024, 0, 1), 0, 1024, 0, 9) &&
              fused_lb(128, 256, 0) == 256 && fused_lb(128, 256, 7) == 256 && fused_lb(320, 256, 1) == 512 && fused_lb(576, 0, 1) == 1024,
              "fused_word: the rule of a launch bound, a CPML form or a hint changed");
static_assert(fused_lds_bytes(4, 0) == 16384 && fused_lds_bytes(8, 7) == 38912, "fused_lds_bytes: the LDS of a workgroup changed");
static_assert(fused_lds_bytes(16, 0) <= 160 * 1024 && fused_lds_bytes(8, 7) <= 160 * 1024, "fused_step_kernel: LDS of a workgroup");

// ---- the launcher (fdtd_capi.hip) ----------------------------------------------------------------------------------------------------
// One launch of the sweep: rows1 = rows per workgroup + the halo row; the word's inputs (matf; lb_req = FDTD_OPT_FUSED_LB; pml_inside;
// mem_hints); lds_pad bytes on top of fused_lds_bytes; then the kernel's arguments.  The launcher runs the instantiation
// <fused_word(...)>, exactly, and returns false (nothing launched) where the list does not hold it.
struct FusedLaunch {
  hipStream_t st;
  int grid_blocks, rows1;
  int matf, lb_req, pml_inside, mem_hints;
  size_t lds_pad;
  GridP g; FieldP a, b; StepP s; MatP m;
  int kbeg, kend, zchunk, pmc_z0, nbx, nby, nbz, xcd_remap;
  const PmlP* pmq;
  int nbz1, k2beg, k2end, ty_a, ty_gap, ex_j0, ex_j1;
};
constexpr FusedWord fused_word(const FusedLaunch& L) { return fused_word(L.matf, 64 * L.rows1, L.lb_req, L.pml_inside, L.mem_hints); }
// the kernel's arguments, in its order
#define FDTD_F1_ARGS(L) (L).g, (L).a, (L).b, (L).s, (L).m, (L).kbeg, (L).kend, (L).zchunk, (L).pmc_z0, (L).nbx, (L).nby, (L).nbz, (L).xcd_remap, (L).pmq, \
                        (L).nbz1, (L).k2beg, (L).k2end, (L).ty_a, (L).ty_gap, (L).ex_j0, (L).ex_j1
// the launcher: the list as case labels on the exact word (in the unit that compiles the kernels); one set of tokens names the
// label and the kernel
#define FDTD_F1_CASE(M, LBV, PV, HV)                                                                                               \
  case fused_key(M, LBV, PV, HV):                                                                                                  \
    hipLaunchKernelGGL((fused_step_kernel<(M) != 0, LBV, PV, HV, (M) == 2>), dim3(L.grid_blocks, 1, 1), dim3(64, L.rows1, 1),      \
                       fused_lds_bytes(L.rows1, PV) + L.lds_pad, L.st, FDTD_F1_ARGS(L));                                           \
    return true;
#define FDTD_F1_LAUNCHER(NAME, LIST)                                                                                               \
  bool NAME(const FusedLaunch& L) {                                                                                                \
    const FusedWord w = fused_word(L);                                                                                             \
    switch (fused_key(w.matf, w.lb, w.pml, w.hint)) { LIST(FDTD_F1_CASE) default: return false; }                                  \
  }

}  // namespace fdtd
