// Two time steps per sweep: what fdtd_capi.hip and fdtd_fused2.hip share (the kernels live in fdtd_kernels2.hpp and are
// compiled in their own translation unit, fdtd_fused2.hip, with the SLP vectorizer off: packed-fp32 code for this kernel
// spends more on moves into aligned register pairs than it saves — 0.810 -> 0.701 ms per step inside one engine,
// profiles/r3q_*).
#pragma once
#include "fdtd_kernels.hpp"

namespace fdtd {

constexpr int kMaxInj = 256;
struct InjP {
  int n;                                   // 0: the node table is not walked (no source alive, no monitor sampling)
  const int* start;                        // [nz + 2] rows of plane k: [start[k], start[k + 1])
  const int4* ent;                         // (i, j, code, index), sorted by plane, sources first, list order kept:
                                           //   code 0 - 2: E-side source node of that component, index into val / val2
                                           //   code 3 - 5: H-side source node (H_x, H_y, H_z), index into val2
                                           //   code 8 + c: a time monitor's sample of component c (0 - 5) of the middle step -> cap[index]
  const float* val;                        // source terms of step n
  const float* val2;                       // source terms of step n+1 (nullptr: not available; then there are no H-side nodes)
  int e2_in_sweep;                         // the E-side terms of step n+1 are added to E^{n+2} by the sweep (else: by the caller behind it)
  float* cap;                              // samples of the middle step (pair_record_kernel)
  // The middle step over the boxes of DFT monitors: H^{n+1/2} for a record at step n (its H terms), E^{n+1} for a record at step
  // n+1 (its E terms) — accumulated behind the sweep, dft_record_dump_kernel.  Boxes of plane k = dlist[dstart[k] .. dstart[k + 1])
  const int* dstart;
  const int* dlist;
  const struct DumpBox* dboxes;
  float* dump;
};
struct DumpBox {
  int lo0, lo1, lo2, nx, ny, nz;           // the monitor's box
  int off[6];                              // offset of the E_x .. H_z block ([nz][ny][nx], the monitor's cell order) in `dump`, -1 = not needed
};
constexpr int kMaxDumps = 8;
// absorber layers (damp_kernel's per-axis factor tables: fb at cell boundaries, fc at cell centres; 1 outside the layers);
// fb[0] == nullptr: none
struct DampT {
  const float* fb[3];
  const float* fc[3];
  int e2;                                  // E^{n+2} is damped inside the sweep (else: by the caller, behind the sources it applies)
};
// the box a clipped launch of the two-step sweep writes: [i0, i1) x [j0, j1) x [k0, k1), i0 and i1 multiples of 4 — the bulk of a
// grid whose shell (CPML slabs + collar, boundary planes of a z-slab rank) is advanced by single steps (fdtd_capi.hip, shell pairs)
struct ClipP { int i0, i1, j0, j1, k0, k1; };
// tile classes of a launch of a materials instantiation: cls[tile] (logical tile index, y fastest) = 0 where the tile holds only the
// background medium — its workgroup runs the plain sweep; 2 (launches that carry dispersive cells) where a row segment of the tile
// holds a dispersive cell, 1 elsewhere — the materials sweep without the ADE lines.  cls == nullptr: the launch's own instantiation everywhere
struct TileClassP { const unsigned char* cls; };
// Dispersive cells in step pairs (round 6; K4 twice per pair): paged storage — one block [3 components][256 cells] of floats per row
// segment (256 cells of one row = one wavefront of the sweep) that holds a dispersive cell, found through dseg.  `cs` holds the
// memory term cc S(Q^n) of the current state at the dispersive cells (0 elsewhere), written by whichever ADE kernel formed Q^n;
// the sweep subtracts it from E^{n+1} in S2 and leaves E^{n+1} of the rows it owns in `e1` for ade2_kernel.  dseg == nullptr: none.
struct DispP {
  const int* dseg;                         // [nz][ny][ceil(nx / 256)]: block of the row segment, -1 = no dispersive cell in it
  const float* cs;                         // cc S(Q^n)
  float* e1;                               // E^{n+1} behind its ADE update
};
// Source terms of a step pair in paged storage (round 6): what TFSF boxes, mode planes, current sheets and other lists of more than
// kMaxInj nodes add to the fields while they inject — one block [3 components][256 cells] per row segment that holds a source node
// (sseg), three arrays filled in front of every pair by list kernels with the operations of point_source_kernel / tfsf_corr_kernel:
// e1 = the E-side terms of step n (added to E^{n+1} in S2, behind the walls, in front of damping and ADE), h2 = the H-side terms of
// step n+1 (added to H^{n+1/2} at the top of S3), e2 = the E-side terms of step n+1 (added to E^{n+2} in S4).  The H-side terms of
// step n act on H^{n-1/2} in front of the sweep, as always.  One term per node and side (the host checks that no two lists meet
// One term per node, side and LAYER: lists that meet on a node (the two polarisation components of a TFSF box with a pol_angle) go to
// different layers in their launch order, and (E + term_0) + term_1 is what the list kernels would have formed one after the other
// (a node only the second list touches adds a zero first).  sseg == nullptr: none.
struct SrcT {                              // (in device memory: a sweep reads it only in the few row segments that hold source nodes —
  const float* e1;                         //  as kernel arguments the eight words cost the sweep 16 scalar registers it spills for)
  const float* h2;
  const float* e2;
  int use_h2, use_e2;                      // a list has H-side / E-side nodes
  const float* e1b;                        // layer 1 (nullptr: no two lists meet)
  const float* h2b;
  const float* e2b;
};
struct SrcP {
  const int* sseg = nullptr;               // [nz][ny][ceil(nx / 256)]: block of the row segment, -1 = no source node in it
  const SrcT* t = nullptr;
};
// ---- the OPT word of fused2_step_kernel<LB, OPT> ---------------------------------------------------------------------------------
// Composed by fused2_opt (fdtd_capi.hip: launch_fused2), matched against the lists of instantiations below by the launchers, decoded
// by the kernel (fdtd_kernels2.hpp).
constexpr int kF2NT = 1;              // non-temporal stores
constexpr int kF2Mat = 2;             // materials: packed medium words + (Ca, Cb) table (m.m4 set)
constexpr int kF2Mon = 4;             // the node table may hold monitor samples
constexpr int kF2Damp = 8;            // absorber layers, damped in registers (dmp.fb[0] set)
constexpr int kF2Clip = 16;           // the launch covers the box `clip` only (never with kF2Damp)
constexpr int kF2Disp = 32;           // the memory terms of dispersive cells are subtracted from E^{n+1} (dp.dseg set; with kF2Mat and kF2NT)
constexpr int kF2Src = 64;            // paged source terms (sr.sseg set; with kF2Mon and kF2NT)
constexpr int kF2WhatifShift = 8, kF2WhatifMask = 15;        // what-if / prefetch variant 1 ... 15 (on top of the word kF2NT alone)
constexpr int kF2NoExj = 4096;        // set by fused2_step_kernel for its tile bodies, never by a launcher: the instantiation has no ninth exchange array
constexpr int kF2Rep = 8192;          // the seam columns of set a are read from the repair array (words of kF2NT, kF2Mat, kF2Damp only)
constexpr int fused2_whatif(int opt) { return (opt >> kF2WhatifShift) & kF2WhatifMask; }
constexpr int fused2_whatif_word(int wv) { return kF2NT | (wv << kF2WhatifShift); }
constexpr bool fused2_rep_word(int opt) { return (opt & ~(kF2NT | kF2Mat | kF2Damp)) == 0; }      // a word that has a kF2Rep form

// The word of a launch, from what launch_fused2 knows: `nt` the non-temporal hint, `mon` the node table is needed, `damp` the grid has
// absorber layers, `disp` / `src` the launch carries dispersive cells (the caller has checked `mat`) / paged source terms, `whatif` the
// variant asked for (0: none; it applies to the word kF2NT alone, at sixteen waves — 13 and 14 at any size), `rep` the repair array is
// read (the caller asks for it on a fused2_rep_word without `clip` only), W waves per workgroup.
constexpr int fused2_opt(bool nt, bool mat, bool mon, bool clip, bool damp, bool disp, bool src, int whatif, bool rep, int W) {
  int opt = (nt ? kF2NT : 0) | (mat ? kF2Mat : 0) | (mon ? kF2Mon : 0) | (clip ? kF2Clip : (damp ? kF2Damp : 0)) |
            (disp ? kF2Disp | kF2NT : 0) | (src ? kF2Src | kF2Mon | kF2NT : 0);
  if (whatif && opt == kF2NT && (W == 16 || whatif == 13 || whatif == 14)) opt = fused2_whatif_word(whatif);
  return opt | (rep ? kF2Rep : 0);
}
// the launch bound of the instantiation that serves `waves` rows per workgroup
constexpr int fused2_lb(int waves, int opt) {
  if ((opt & kF2Rep) || fused2_whatif(opt)) return 1024;
  if (waves <= 8) return 512;
  return (waves <= 12 && !(opt & (kF2Src | kF2Disp))) ? 768 : 1024;
}

// The instantiations that exist: one list of X(LB, OPT) per translation unit (they compile side by side).  Each unit expands its list
// into its launcher's case labels (FDTD_F2_LAUNCHER), fused2_instantiated expands all of them: a word outside them is refused, never
// mapped to a neighbour.
#define FDTD_F2_AT512(X, O) X(512, (O))
#define FDTD_F2_AT768(X, O) X(768, (O))
#define FDTD_F2_AT1024(X, O) X(1024, (O))
#define FDTD_F2_ANY_NT(AT, X, O) AT(X, O) AT(X, (O) | kF2NT)
#define FDTD_F2_ANY_MAT(AT, X, O) FDTD_F2_ANY_NT(AT, X, O) FDTD_F2_ANY_NT(AT, X, (O) | kF2Mat)
#define FDTD_F2_ANY_MON(AT, X, O) FDTD_F2_ANY_MAT(AT, X, O) FDTD_F2_ANY_MAT(AT, X, (O) | kF2Mon)
// fdtd_fused2.hip: the whole grid, with / without absorber layers; and the deferred-seam forms (sixteen-wave instantiations only)
#define FDTD_F2_BASE_AT(AT, X) FDTD_F2_ANY_MON(AT, X, 0) FDTD_F2_ANY_MON(AT, X, kF2Damp)
#define FDTD_F2_LIST_REP(X) FDTD_F2_ANY_MAT(FDTD_F2_AT1024, X, kF2Rep) FDTD_F2_ANY_MAT(FDTD_F2_AT1024, X, kF2Rep | kF2Damp)
#define FDTD_F2_LIST_BASE(X) FDTD_F2_BASE_AT(FDTD_F2_AT512, X) FDTD_F2_BASE_AT(FDTD_F2_AT768, X) FDTD_F2_BASE_AT(FDTD_F2_AT1024, X)
// fdtd_fused2c.hip: clipped to the bulk of a shell pair
#define FDTD_F2_LIST_CLIP(X) FDTD_F2_ANY_MON(FDTD_F2_AT512, X, kF2Clip) FDTD_F2_ANY_MON(FDTD_F2_AT768, X, kF2Clip) FDTD_F2_ANY_MON(FDTD_F2_AT1024, X, kF2Clip)
// fdtd_fused2d.hip: dispersive cells — materials + ADE, non-temporal stores; with / without the monitor table; whole grid, absorber layers or clipped
#define FDTD_F2_DISP_MON(AT, X, O) AT(X, kF2Disp | kF2Mat | kF2NT | (O)) AT(X, kF2Disp | kF2Mat | kF2NT | kF2Mon | (O))
#define FDTD_F2_DISP_AT(AT, X) FDTD_F2_DISP_MON(AT, X, 0) FDTD_F2_DISP_MON(AT, X, kF2Damp) FDTD_F2_DISP_MON(AT, X, kF2Clip)
#define FDTD_F2_LIST_DISP(X) FDTD_F2_DISP_AT(FDTD_F2_AT512, X) FDTD_F2_DISP_AT(FDTD_F2_AT1024, X)
// fdtd_fused2s.hip: paged source terms — monitor table, non-temporal stores; with / without materials; the materials ones also with
// the dispersive cells' memory terms; whole grid, absorber layers or clipped
#define FDTD_F2_SRC_MAT(AT, X, O) AT(X, kF2Src | kF2Mon | kF2NT | (O)) AT(X, kF2Src | kF2Mon | kF2NT | kF2Mat | (O))
#define FDTD_F2_SRC_DISP(AT, X, O) AT(X, kF2Src | kF2Mon | kF2NT | kF2Mat | kF2Disp | (O))
#define FDTD_F2_SRC_AT(AT, X)                                                                          \
  FDTD_F2_SRC_MAT(AT, X, 0) FDTD_F2_SRC_MAT(AT, X, kF2Damp) FDTD_F2_SRC_MAT(AT, X, kF2Clip)              \
  FDTD_F2_SRC_DISP(AT, X, kF2Clip) FDTD_F2_SRC_DISP(AT, X, 0) FDTD_F2_SRC_DISP(AT, X, kF2Damp)
#define FDTD_F2_LIST_SRC(X) FDTD_F2_SRC_AT(FDTD_F2_AT512, X) FDTD_F2_SRC_AT(FDTD_F2_AT1024, X)
// fdtd_fused2w.hip: the what-if and prefetch variants of the vacuum sweep
#define FDTD_F2_WV(X, WV) X(1024, fused2_whatif_word(WV))
#define FDTD_F2_LIST_WHATIF(X)                                                                                        \
  FDTD_F2_WV(X, 1) FDTD_F2_WV(X, 2) FDTD_F2_WV(X, 3) FDTD_F2_WV(X, 4) FDTD_F2_WV(X, 5) FDTD_F2_WV(X, 6) FDTD_F2_WV(X, 7) FDTD_F2_WV(X, 8) \
  FDTD_F2_WV(X, 9) FDTD_F2_WV(X, 10) FDTD_F2_WV(X, 11) FDTD_F2_WV(X, 12) FDTD_F2_WV(X, 13) FDTD_F2_WV(X, 14) FDTD_F2_WV(X, 15)
#define FDTD_F2_LIST_OWN(X) FDTD_F2_LIST_REP(X) FDTD_F2_LIST_BASE(X)
#define FDTD_F2_LIST_ALL(X) FDTD_F2_LIST_OWN(X) FDTD_F2_LIST_CLIP(X) FDTD_F2_LIST_DISP(X) FDTD_F2_LIST_SRC(X) FDTD_F2_LIST_WHATIF(X)
// (LB, OPT) as one switch value (a pair listed twice is a duplicate case label)
constexpr int fused2_key(int lb, int opt) { return opt * 2048 + lb; }
constexpr bool fused2_instantiated(int lb, int opt) {
  switch (fused2_key(lb, opt)) {
#define FDTD_F2_X(LBV, OV) case fused2_key(LBV, OV):
    FDTD_F2_LIST_ALL(FDTD_F2_X)
#undef FDTD_F2_X
      return true;
    default: return false;
  }
}
// every word launch_fused2 can form — clip excludes the absorber bit, dispersive cells need materials, a what-if variant and the
// repair array apply where fused2_opt / fused2_rep_word say — has its instantiation: a new bit without one stops the build, not a run
constexpr bool fused2_words_instantiated() {
  for (int W = 4; W <= 16; ++W)
    for (int in = 0; in < 128; ++in) {
      const bool nt = in & 1, mat = in & 2, mon = in & 4, clip = in & 8, damp = in & 16, disp = in & 32, src = in & 64;
      if ((clip && damp) || (disp && !mat)) continue;
      for (int wv = 0; wv <= 15; ++wv) {
        const int opt = fused2_opt(nt, mat, mon, clip, damp, disp, src, wv, false, W);
        if (wv && !fused2_whatif(opt)) continue;        // (the variant does not apply here: the word of wv = 0)
        if (!fused2_instantiated(fused2_lb(W, opt), opt)) return false;
        const int rep = fused2_opt(nt, mat, mon, clip, damp, disp, src, wv, true, W);
        if (!clip && fused2_rep_word(opt) && !fused2_instantiated(fused2_lb(W, rep), rep)) return false;
      }
    }
  return true;
}
static_assert(fused2_words_instantiated(), "fused2_opt forms a word that no list of instantiations holds");

// exchange arrays of a workgroup of `waves` rows ([.][waves][64] float4 of dynamic LDS): H1_x H1_z | H2_x H2_z | E1_x E1_z twice, and — in
// most instantiations (fused2_exj) — E_x of the next plane for the row below (fdtd_kernels2.hpp, EXJ)
#if !defined(FDTD_NO_EXJ)
#define FDTD_NO_EXJ 0       // (1: a build without it — the A/B of the other instantiations, variants/libfdtd_hip_noexj.so)
#endif
// (lb: the instantiation's launch bound, 512 / 768 / 1024 threads for <= 8 / <= 12 / <= 16 waves; opt: its OPT word.  What
//  fused2_step_kernel asks about its own word — the what-if variants decide EXJ from their number in the tile body, and count below)
constexpr bool fused2_exj(int lb, int opt) { return !FDTD_NO_EXJ && (opt & kF2Damp) == 0 && !(lb == 512 && (opt & kF2Mat) != 0); }
// (what-if variants: 13 has the ninth array; the prefetch variants 10 - 12 keep six exchange arrays + the 3 / 2 / 3 arrays of the next
//  plane that travel through LDS; the others keep eight)
constexpr int fused2_xch_arrays(int lb, int opt) {
  const int wv = fused2_whatif(opt);
  if (wv) return wv == 13 ? 9 : ((wv >= 10 && wv <= 12) ? 6 + (wv == 11 ? 2 : 3) : 8);
  return fused2_exj(lb, opt) ? 9 : 8;
}
// dynamic LDS of a launch of fused2_step_kernel<lb, opt> with `waves` rows per workgroup (+ the absorber layers' x factors, + the (Ca, Cb)
// table: a what-if word has neither bit)
constexpr size_t fused2_lds_bytes(int lb, int opt, int waves) {
  return ((size_t)fused2_xch_arrays(lb, opt) * waves * 64 + ((opt & kF2Damp) ? 2 * 64 : 0)) * sizeof(float4) + ((opt & kF2Mat) ? (size_t)kMaxMedia * sizeof(float2) : 0);
}
// (everything a workgroup of the sweep keeps in LDS is in this one dynamic allocation — no static arrays in the tile bodies, which a
//  kernel of several bodies would hold once per body — so the 160 KB of a gfx950 CU bound it here, at compile time)
static_assert(fused2_lds_bytes(1024, kF2NT | kF2Mat | kF2Mon | kF2Clip | kF2Disp | kF2Src, 16) <= 160 * 1024 && fused2_lds_bytes(1024, kF2Mat | kF2Damp, 16) <= 160 * 1024 &&
              2 * fused2_lds_bytes(512, kF2NT, 8) <= 160 * 1024 && 2 * fused2_lds_bytes(512, kF2Mat | kF2Damp, 8) <= 160 * 1024,
              "fused2_step_kernel: LDS of a workgroup (two per CU for eight waves)");
// the bytes of every listed instantiation, pinned in bare numbers (independent of the names above, and of fused2_xch_arrays): a what-if
// word at sixteen waves by its variant, every other word by its exchange arrays (nine with EXJ), absorber factors and table
constexpr bool fused2_lds_pinned(int lb, int opt) {
  const int wv = fused2_whatif(opt), w = lb / 64;
  if (wv) return fused2_lds_bytes(lb, opt, 16) == ((size_t)(wv == 13 ? 9 : ((wv >= 10 && wv <= 12) ? 6 + (wv == 11 ? 2 : 3) : 8)) * 16 * 64) * sizeof(float4);
  return fused2_lds_bytes(lb, opt, w) == ((size_t)(fused2_exj(lb, opt) ? 9 : 8) * w * 64 + ((opt & 8) ? 2 * 64 : 0)) * sizeof(float4) + ((opt & 2) ? (size_t)kMaxMedia * sizeof(float2) : 0);
}
#define FDTD_F2_X(LBV, OV) && fused2_lds_pinned(LBV, OV)
static_assert(true FDTD_F2_LIST_ALL(FDTD_F2_X), "fused2_lds_bytes: the LDS of a listed instantiation changed");
#undef FDTD_F2_X
constexpr int kMaxCap = 1024;
constexpr int kSeamArrays = 13;  // of step one: H1_y, H1_z, E1_x, E1_y, E1_z [c-1], E1_y, E1_z [c]; of step two: H2_x [c-1], H2_y, H2_z [c-2], H2_x, H2_y, H2_z [c]
                                 // (c = first column of the right tile)

// host-side launchers (fdtd_fused2.hip)
void launch_inject_values(hipStream_t st, float* val, const float* w_re, const float* w_im, const float2* wave,
                          long long step, int n);
// One launch of the sweep.  waves = rows per workgroup (W - 3 of them written); opt: the word above — the launchers run the
// instantiation <fused2_lb(waves, opt), opt>, exactly, and return false (nothing launched) where no list holds it.
struct Fused2Launch {
  hipStream_t st;
  int waves, opt, grid_blocks;
  GridP g; FieldP a, b; StepP s; MatP m;
  int zchunk, nbx, nby, nbz, xcd_remap;
  InjP inj; float* seam; DampT dmp; ClipP clip; TileClassP tcl; DispP dp; SrcP sr;
};
// the kernel's arguments, in its order
#define FDTD_F2_ARGS(L) (L).g, (L).a, (L).b, (L).s, (L).m, (L).zchunk, (L).nbx, (L).nby, (L).nbz, (L).xcd_remap, (L).inj, (L).seam, (L).dmp, (L).clip, (L).tcl, (L).dp, (L).sr
// a unit's launcher: its list as case labels on the exact pair (in a unit that includes fdtd_kernels2.hpp)
#define FDTD_F2_CASE(LBV, OV)                                                                                                      \
  case fused2_key(LBV, OV):                                                                                                        \
    hipLaunchKernelGGL((fused2_step_kernel<LBV, OV>), dim3(L.grid_blocks, 1, 1), dim3(64, L.waves, 1), fused2_lds_bytes(LBV, OV, L.waves), L.st, \
                       FDTD_F2_ARGS(L));                                                                                           \
    return true;
#define FDTD_F2_LAUNCHER(NAME, LIST)                                                                                               \
  bool NAME(const Fused2Launch& L) {                                                                                               \
    switch (fused2_key(fused2_lb(L.waves, L.opt), L.opt)) { LIST(FDTD_F2_CASE) default: return false; }                            \
  }
// picks the unit from the word: paged sources fdtd_fused2s.hip, what-if fdtd_fused2w.hip, dispersive fdtd_fused2d.hip, clipped
// fdtd_fused2c.hip, the others its own (each in its own translation unit: they compile side by side)
bool launch_fused2_step(const Fused2Launch& L);
bool launch_fused2_step_src(const Fused2Launch& L);
bool launch_fused2_step_whatif(const Fused2Launch& L);
bool launch_fused2_step_disp(const Fused2Launch& L);
bool launch_fused2_step_clip(const Fused2Launch& L);
void launch_inject_table(hipStream_t st, float* tab, long long stride, long long off, const float* w_re, const float* w_im,
                         const float2* wave, long long n_steps, int n);
constexpr int kPairMons = 4;
struct PairRecP {
  int n_mon;
  int pre_done;                  // E^n and the first H half-sample of records at step n were taken in front of the sweep
  BoxP box[kPairMons];
  int nc[kPairMons];
  int comp[kPairMons][6];
  int cap_off[kPairMons];
  float* out_n[kPairMons];       // the record of step n / n+1, nullptr = the monitor does not record then
  float* out_m[kPairMons];
};
void launch_pair_record(hipStream_t st, const PairRecP& r, long long max_cells, const GridP& g, const FieldP& a, const FieldP& b,
                        const float* cap);
// acc[f][slot][cell] += dump[cell] * phase[f]: terms of a DFT record from the sweep's copy of the middle step (the operations of
// dft_record_multi_kernel); n entries: (slot, offset into dump)
struct DftDumpP { int n; int slot[3]; int off[3]; };
void launch_dft_record_dump(hipStream_t st, const DftDumpP& r, const float* dump, float2* acc, long long cells, long long fstride,
                            const float2* phase, int nf);
// (inj: the seam kernel adds the E-side source terms of step n+1 when the sweep did — inj.e2_in_sweep)
// (rep: deferred seam repair — the repaired values go into the compact array, not into set b)
void launch_seams(hipStream_t st, const GridP& g, const FieldP& b, const StepP& s, const MatP& m, const float* seam,
                  int n_seams, const DampT& dmp, const ClipP& clip, const InjP& inj, const SrcP& sr = SrcP{}, float* rep = nullptr);
// deferred seam repair (fdtd_kernels2.hpp): the compact array [seam][kRepArrays][nz][ny] lies behind the scratch arrays of the seam buffer
constexpr int kRepArraysHost = 7;
inline size_t seam_scratch_floats(const GridP& g, int n_tiles_x) { return (size_t)n_tiles_x * kSeamArrays * (size_t)(g.nz + 2) * (size_t)g.ny; }
inline size_t seam_rep_floats(const GridP& g, int n_tiles_x) { return (size_t)n_tiles_x * kRepArraysHost * (size_t)g.nz * (size_t)g.ny; }
// scatters the repair array into the seam columns of set b
void launch_seam_flush(hipStream_t st, const GridP& g, const FieldP& b, const float* rep, int n_seams);

}  // namespace fdtd
