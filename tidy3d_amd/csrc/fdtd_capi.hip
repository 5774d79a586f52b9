// libfdtd_hip.so — host side of the C ABI declared in include/fdtd_hip.h.
// Owns device memory, HIP streams/events and the RCCL communicator of one z-slab solver.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "../../include/fdtd_hip.h"
#include "fdtd_kernels.hpp"
#include "fdtd_fused.hpp"
#include "fdtd_fused2.hpp"
#include "fdtd_strip.hpp"
#include "fdtd_shell2_host.hpp"
#include "fdtd_aniso.hpp"
#include "fdtd_modulation.hpp"
#include "fdtd_conformal.hpp"
#include "fdtd_nonlinear.hpp"
#include "fdtd_near_field.hpp"
#include "fdtd_flux_time.hpp"
#include "fdtd_field_time.hpp"
#include "fdtd_field_dft.hpp"
#include "fdtd_lattice_dft.hpp"
#include "fdtd_lattice_flux.hpp"
#include "fdtd_raster.hpp"

using namespace fdtd;

namespace {

thread_local std::string g_create_error;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct PmlAxisDev {
  int n_lo = 0, n_hi = 0, n = 0;   // true layer counts (what the slab kernels visit)
  // membership of the psi arrays (same on the E and the H side, fdtd_kernels.hpp PmlAxisP): index ia is
  // held when ia < lo or ia >= hi0; along x both are multiples of 4 cells
  int lo = 0, hi0 = 0, ns = 0;
  float4 *ce4 = nullptr, *ch4 = nullptr;                       // {1/kappa - 1, b, c, 0} per index
  float *kv_e = nullptr, *b_e = nullptr, *c_e = nullptr, *kv_h = nullptr, *b_h = nullptr, *c_h = nullptr;
  // psi arrays: [comp slot 0/1]
  float* psi_e[2] = {nullptr, nullptr};
  float* psi_h[2] = {nullptr, nullptr};
  float* psi_h2[2] = {nullptr, nullptr};   // write set of the in-sweep CPML (ping-pong), lazily allocated
  float* psi_e2[2] = {nullptr, nullptr};   // write set of the E side for shell2_step_kernel (two steps per sweep carry psi: both sides ping-pong), lazily allocated
  float* psi_ht[2] = {nullptr, nullptr};   // temporary sets: the middle step of the z holes of a shell2 pair (single steps beside boxes that
  float* psi_et[2] = {nullptr, nullptr};   // still read the old values), lazily allocated
  size_t psi_count = 0;                    // entries per psi array
  size_t psi_plane = 0;                    // entries of one z-plane of it (x, y axes: the H-side arrays carry one more, the ghost slot)
  // the six sets by number, in the order they are allocated (the first two by fdtd_set_pml, the others lazily: ensure_psi_sets),
  // and the entries each array of a set holds
  enum Set { kE, kH, kH2, kE2, kHt, kEt, kSets };
  float** set(int s) { float** const v[kSets] = {psi_e, psi_h, psi_h2, psi_e2, psi_ht, psi_et}; return v[s]; }
  size_t set_count(int s) const { return psi_count + (s == kH || s == kH2 || s == kHt ? psi_plane : 0); }
};

struct AdeGroup {
  int comp;
  int k0 = 0, k1 = 0;              // planes [k0, k1) that hold its cells: launches over other plane ranges are skipped
  std::vector<long long> plane_off;  // sorted lists: entries of plane k are [plane_off[k], plane_off[k + 1]); empty = unsorted
  bool strict = false;               // sorted and no cell listed twice
  long long n;
  uint32_t* cell;
  float* e_old;
  float2* q;
  AdeP p;
  uint32_t* qoff = nullptr;        // slot of entry t in the paged arrays (Disp)
};

// Which block of paged storage a row segment (256 cells of one row) owns: the map both pagings (Disp, SrcPaged) address their
// arrays by, on the device for the kernels and on the host for the tile classes and the shell's boxes.  seg_map_build lays it out.
struct SegMap {
  int* dev = nullptr;              // [nz][ny][nbx]: block of the row segment, -1 = none
  std::vector<int> host;           // the same (empty: not built)
  int n_blocks = 0;
  // does a row segment of planes k0 .. k1, rows j0 .. j1, x-tiles t0 .. t1 (inclusive; clamped to the grid here) own a block?
  bool any(const GridP& g, int k0, int k1, int j0, int j1, int t0, int t1) const {
    const int nbx = (g.nx + 255) / 256;
    if (host.empty()) return false;
    for (int k = std::max(k0, 0); k <= std::min(k1, g.nz - 1); ++k)
      for (int j = std::max(j0, 0); j <= std::min(j1, g.ny - 1); ++j)
        for (int t = std::max(t0, 0); t <= std::min(t1, nbx - 1); ++t)
          if (host[((size_t)k * g.ny + j) * nbx + t] >= 0) return true;
    return false;
  }
};

// Dispersive cells in step pairs (round 6; fdtd_fused2.hpp DispP).  What a two-step sweep needs of the ADE update of its first step is
// the memory term cc S(Q^n) at the dispersive cells — known before the sweep starts.  Once a run may take such pairs it is kept in
// paged storage (`cs`: one block per row segment that holds a dispersive cell) by every ADE kernel of this handle; the sweep subtracts
// it and leaves E^{n+1} in `e1`; ade2_kernel behind the sweep advances the pole states two steps.  The lists stay what they were.
struct Disp {
  int state = 0;                   // 0 = not tried, 1 = ready, -1 = this problem cannot
  SegMap seg;                      // the row segments that hold a dispersive cell (DispP::dseg)
  float* cs = nullptr;             // [seg.n_blocks][3][256]
  float* e1 = nullptr;
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};     // bounding box of the dispersive cells [lo, hi)
  long long pairs = 0;             // pairs of the last run whose sweep carried the ADE update of its first step
};

// ---- whole-grid node lists: structure-of-arrays lists of the nodes of one field component, applied by small kernels around every
// single step (h_side_terms / e_side_terms say what a whole-grid list is, who applies it and who refuses it).  Four kinds:
struct ListHead { int comp; long long n; uint32_t* cell; };      // the field component whose nodes are listed, how many, which [n]
struct AnisoGroup : ListHead {      // fdtd_aniso.hpp: the off-diagonal coupling of E component `comp` inside fully anisotropic bodies
  uint32_t* nbr;
  float *w_new, *w_old, *old, *delta;
  uint8_t* wrap;                    // [8n] wrap codes of the slots (fdtd_add_aniso_bloch), nullptr = none: read by fdtd_run_bloch only
};
struct ModGroup : ListHead {        // fdtd_modulation.hpp: the nodes of E component `comp` inside time-modulated media
  float *ca, *eps_bar, *s_bar, *old;
  float2 *d_eps, *d_s;
  double w_eps, w_sig;              // phase advance per time step (rad) of the permittivity / conductivity modulation
};
struct ConformalGroup : ListHead {  // fdtd_conformal.hpp: the faces of H component `comp` (3..5) cut by a PEC surface
  uint32_t* nbr;                    // [4][n] edge nodes, kNoNode = none
  float* d;                         // [4][n]
};
struct NonlinearGroup : ListHead {  // fdtd_nonlinear.hpp: the nodes of E component `comp` inside Kerr media
  uint32_t* nbr;                    // [8][n] the four E_b and the four E_c nodes around each node, kNoNode = none
  float *den0, *chi3;               // [n] eps_bar + s_bar, chi3
  float *old, *i_old, *lin, *next;  // [n] E^n, I^n, E_lin, the iterate being formed
};
// One row per kind, in the order the step-pair off-reason names them; every kind keeps single steps and one GPU.  `early`: fdtd_add_*
// and fdtd_comm_init refuse the kind on z-slabs already — the fully anisotropic lists are refused by Run::setup / BlochRun::setup
// only (on record, not by design).  `bloch_lists`: what a Bloch pair's error calls the lists both handles must carry alike (linear
// updates with real coefficients: each part is patched by its own); nullptr = refused with Bloch boundaries (Kerr: not linear).
enum ListKind { kAniso, kModulation, kConformal, kNonlinear, kListKinds };
constexpr struct { const char* noun; int f2_off; bool early; const char* bloch_lists; } kListKind[kListKinds] = {
    {"fully anisotropic media", FDTD_F2_OFF_ADE, false, "fully anisotropic lists"},
    {"time-modulated media", FDTD_F2_OFF_MODULATION, true, "time-modulation lists"},
    {"PEC-conformal boundaries", FDTD_F2_OFF_CONFORMAL, true, "PEC-conformal lists"},
    {"nonlinear media", FDTD_F2_OFF_NONLINEAR, true, nullptr}};

// The points of one side (E or H components) of a point-source list (point_source_kernel).  PointSide and TfsfList name what the paged
// source terms need of a side alike: n, cell, comp, soff, layer (for_each_source_side).
struct PointSide {
  long long n = 0;
  int k0 = 0, k1 = 0;              // planes [k0, k1) that hold its points
  int32_t* comp = nullptr;
  uint32_t* cell = nullptr;
  float *wre = nullptr, *wim = nullptr;
  float2* wave = nullptr;
  uint32_t* soff = nullptr;        // slots of the nodes in the paged source terms (SrcPaged)
  int layer = 0;                   // their layer
  std::vector<int32_t> host_comp;  // host copies of the nodes (the two-step sweep applies them in-kernel)
  std::vector<uint32_t> host_cell;
};
struct PointSrc {
  long long n_steps = 0;
  PointSide e, h;
  const PointSide& side(bool e_side) const { return e_side ? e : h; }
  bool has_nodes() const { return e.n || h.n; }
  bool alive(long long n) const { return has_nodes() && n < n_steps; }       // the list injects at step n
  bool e_due(long long n) const { return e.n && n < n_steps; }               // its E side injects at step n
};

// correction list of one side (E or H) of a TFSF box, grouped by target node (tfsf_corr_kernel)
struct TfsfList {
  int k0 = 0, k1 = 0;              // planes [k0, k1) that hold its target nodes
  long long n = 0;                 // target nodes
  int32_t *comp = nullptr, *start = nullptr, *aux = nullptr;
  uint32_t* cell = nullptr;
  float* w = nullptr;
  uint32_t* soff = nullptr;        // slots of the target nodes in the paged source terms (SrcPaged)
  int layer = 0;                   // their layer
};

struct Tfsf {
  int n_aux = 0, src_cell = 0;
  float *ae = nullptr, *be = nullptr, *ah = nullptr, *bh = nullptr, *e1 = nullptr, *h1 = nullptr, *wave = nullptr;
  float *e1c = nullptr, *h1c = nullptr;   // replica advanced on the comm stream (pipelined z-slab schedule)
  long long n_steps = 0;
  TfsfList e, h;
};

// what `data` holds and what becomes of it: records or accumulators of the whole box, read back as they are (fdtd_add_monitor); a
// ring of records that ring_drain reduces to one flux value each (fdtd_flux_time.hpp) or gathers onto the kept nodes
// (fdtd_field_time.hpp); DFT accumulators on the kept nodes alone (fdtd_field_dft.hpp), or on the sampling lattice of a projection
// surface alone (fdtd_lattice_dft.hpp: the tables of `dp` then hold kLatticeTaps taps per node and axis)
enum class MonForm { Whole, FluxRing, SparseRing, SparseDft, LatticeDft };
enum { kBytesTotal, kBytesRecords, kBytesResult, kBytesTables };      // the figures of fdtd_get_monitor_bytes

struct Monitor {
  int kind = 0;                    // FDTD_MON_TIME / FDTD_MON_DFT: how every schedule treats the monitor, whatever its form
  MonForm form = MonForm::Whole;
  std::vector<int> comps;
  BoxP box{};
  std::vector<long long> steps;
  size_t next = 0;                 // next entry of `steps` to record
  int nf = 0;
  float2 *phase_e = nullptr, *phase_h = nullptr;   // [n_rec][nf]
  void* data = nullptr;            // Whole: [n_rec][comps][box] floats / [nf][comps][box] float2; rings: `ring` records (slot = record
  size_t data_bytes = 0;           // index mod ring); SparseDft, LatticeDft: float2 [nf][kept nodes]
  long long cells = 0;
  int64_t held[4] = {0, 0, 0, 0};  // device memory the monitor holds, by kBytes*: taken where it is allocated (took)
  int64_t mark = 0;                // h->stats.device_bytes when the last of them was taken
  size_t ring = 0;                 // records the staging buffer holds (0: no ring)
  size_t reduced = 0;              // records [0, reduced) are in `result`, their slots zero again
  size_t result_bytes = 0;         // what fdtd_get_monitor returns of a ring monitor: the series / the gathered array
  FluxMonP fp{};                   // FluxRing: addresses and shapes of its tables
  FieldTimeP gp{};                 // SparseRing
  FieldDftP dp{};                  // SparseDft, LatticeDft
  LatticeFluxP lp{};               // LatticeDft with integration weights (fdtd_set_lattice_flux_weights): what fdtd_lattice_flux reduces
  bool has_flux = false;
  float* result() const { return form == MonForm::FluxRing ? fp.result : gp.out; }
  long long slot(size_t rec) const { return (long long)(ring ? rec % ring : rec); }
};
inline bool has_ring(const Monitor& m) { return m.form == MonForm::FluxRing || m.form == MonForm::SparseRing; }
// the forms that read their whole box on one handle: not on z-slab handles, not with Bloch boundaries
inline bool needs_whole_grid(const Monitor& m) { return m.form != MonForm::Whole; }
// what the schedules ask of a monitor: does it record like a running DFT over its box (E^n at the pre point, H^{n+1/2} at the post
// point, the middle step of a pair from the sweep's dump)?  The whole-box DFT monitor and the sparse one alike.
inline bool records_as_dft(const Monitor& m) { return m.kind == FDTD_MON_DFT; }

// node table of one kind of step pair of the two-step sweep: the E-side source nodes and the nodes small time monitors
// sample of the middle step (InjP), for one set of recording monitors
struct F2Table {
  bool with_sources = true;        // the source nodes are listed (false: the table of a pair whose source lists are all spent)
  std::vector<int> mons;           // time monitors whose middle-step samples the sweep copies out (ascending)
  std::vector<int> cap_off;        // their offsets into the sample buffer
  std::vector<int> dfts;           // DFT monitors that record at the first (flag 1) / middle (flag 2) step: the sweep copies
  std::vector<int> dft_when;       // H^{n+1/2} / E^{n+1} over their boxes out
  std::vector<std::array<int, 6>> dft_off;     // offsets of their E_x .. H_z blocks in the dump buffer (-1: not needed)
  int* start = nullptr;
  int4* ent = nullptr;
  int *dstart = nullptr, *dlist = nullptr;
  DumpBox* dboxes = nullptr;
  long long dump_floats = 0;
};
struct F2Plan {                    // one step pair: the monitors that record at its first or middle step
  std::vector<int> mons;           // small time monitors
  std::vector<int> dfts;           // DFT monitors recording at the first and / or the middle step
  std::vector<int> dft_when;       // bit 0: at step n, bit 1: at step n + 1
};

}  // namespace

// Paged source terms (round 6; fdtd_fused2.hpp SrcP): step pairs while a TFSF box, a mode plane, a current sheet — any list the
// two-step sweep's node table cannot hold — injects.  In front of every such pair list kernels leave what the lists would add at steps
// n (E side), n + 1 (H side) and n + 1 (E side) in three paged arrays; the sweep, the seam kernel and the shell's boxes add them.
struct SrcPaged {
  int state = 0;                   // 0 = not tried, 1 = ready, -1 = this problem cannot (two lists meet on a node, ...)
  SegMap seg;                      // the row segments that hold a source node (SrcP::sseg)
  float *e1 = nullptr, *h2 = nullptr, *e2 = nullptr;     // [seg.n_blocks][3][256]: layer 0
  float *e1b = nullptr, *h2b = nullptr, *e2b = nullptr;  // layer 1: lists that meet an earlier list on a node (nullptr: none does)
  bool any_h = false;              // a list has H-side nodes
  long long pairs = 0;
  SrcT* tab = nullptr;             // the arrays' addresses, in device memory (SrcP::t)
  size_t n_psrc = 0, n_tfsf = 0;   // the list counts spg_setup saw: lists added since then make the tables stale (spg_release)
};

struct FdtdSolver {
  FdtdConfig cfg{};
  GridP g{};
  std::string err;
  std::vector<DevBuf> bufs;          // everything hipMalloc'ed (freed in destroy)
  float* fbase[6] = {};              // allocation base (ghost plane -1)
  FieldP f{};                        // interior plane 0 of the CURRENT field set
  float* fbase2[6] = {};             // second set for the fused (ping-pong) sweep, lazily allocated
  FieldP f2{};
  float* fbase3[6] = {};             // third set: the middle step of a shell pair over the shell (lazily allocated)
  FieldP f3{};
  float* step_base[2] = {};          // 1/primal_z, 1/dual_z with one ghost entry on each side
  size_t field_bytes = 0;
  float *ip[3] = {}, *idl[3] = {};
  uint32_t* mat4 = nullptr;          // packed material words (interior plane 0), nullptr = uniform
  uint32_t* mat4b = nullptr;         // wide layout (more than 1023 media): the second word per cell; mat4 then holds E_x | E_y << 16
  uint32_t* roww = nullptr;          // row-segment words [nz][ny][ceil(nx / 256)]
  std::vector<uint32_t> roww_host;   // host copy of them: the tile classes of the two-step sweep are derived from it (tile_classes)
  struct TileClasses { int W, zc; ClipP box; int nbx, nby, nbz; unsigned char* dev; long long n_bg, n_all; bool disp, src; };
  std::vector<TileClasses> tile_cls; // one entry per launch shape met so far
  int tile_split = -1;               // FDTD_OPT_TILE_SPLIT: background-only tiles on the plain instantiation: -1 = default (where >= 25 % of the tiles are), 0 = never, 1 = always
  float2* lut = nullptr;
  int n_media = 0;
  float ca1 = 1.f, cb1 = 0.f;
  std::vector<float> cb_host;
  PmlAxisDev pml[3];
  // absorber layers: per-axis damping tables (identity tables of length N for axes without layers)
  float *damp_fb[3] = {}, *damp_fc[3] = {};
  int damp_lo[3] = {0, 0, 0}, damp_hi[3] = {0, 0, 0};   // layers: index < lo or index >= hi
  bool has_damp = false;
  std::vector<AdeGroup> ade;
  Disp disp;
  SrcPaged spg;
  std::map<std::array<int, 6>, int> box_paged;       // Shell2P::paged of the shell's boxes met so far (cleared when either paging is set up)
  int spg_on = -1;                   // FDTD_OPT_SRC_PAGED: -1 / 1 = default (on), 0 = off (single steps / z holes while such lists inject, round 5)
  // (19: the vacuum sweep without its one-lane stores into the seam scratch)
  // (16 - 18, any plain sixteen-wave pair: 16 = no seam_kernel launch, 17 = 16 + the sweep's edge lanes read the repair array, 18 = seam_kernel stores into the repair array)
  int whatif = 0;                    // FDTD_OPT_WHATIF: a what-if instantiation of the vacuum two-step sweep (fdtd_kernels2.hpp; wrong results, meaningful times)
  int disp_on = -1;                  // FDTD_OPT_DISP: dispersive cells inside the two-step sweeps: -1 = default (on), 0 = off (their planes as z holes, round 5)
  std::vector<AnisoGroup> aniso;
  std::vector<ModGroup> modulation;
  std::vector<ConformalGroup> conformal;
  std::vector<NonlinearGroup> nonlinear;   // at most one list per E component
  int nonlinear_iters = 0;           // fixed-point iterations per step, the same for every list of the handle
  std::vector<PointSrc> psrc;
  std::vector<Tfsf> tfsf;
  std::vector<Monitor> mons;
  hipStream_t stream = nullptr, comm_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> kev;       // per-launch timing events (FDTD_FLAG_TIME_KERNELS)
  std::vector<int> kev_kind;
  double* energy_dev = nullptr;      // [0] = total, [1 .. 1 + kEnergyBlocks) = per-workgroup partial sums
  int decay_every = 0;
  double shutoff = 0.0;
  long long decay_ref = 0;
  double energy_max = 0.0;
  long long step = 0;
  FdtdStats stats{};
  int zchunk = 2;
  int zchunk_f = 16;                 // planes marched per workgroup by the fused sweep (8 without in-sweep CPML: launch_fused_range)
  int last_zc = 0;
  int rows_f = 3;                    // rows per workgroup of the fused sweep (+1 halo wave = 256 threads:
                                     // ~150 VGPRs without spills, 3 workgroups per CU; measured best, profiles/r01g)
  // tile order of the sweep: -1 = default (runs of kTileRun tiles per XCD), 0 = plain, 1 = one contiguous eighth of
  // the tiles per XCD (round 1), G > 1 = runs of G tiles per XCD; measurements at launch_fused_range
  int xcd_remap = -1;
  int fused_lb = 0;                  // 0 = by workgroup size, else forced __launch_bounds__ variant
  // axis mask of the CPML recursions folded into the fused sweep (single GPU): 0 = slab kernels,
  // 6 = y and z, 7 = all.  Measured on 512^3 + 12-layer PML (profiles/r01h_pml_placement.txt): the
  // extra live registers drop the sweep from 3 to 2 (mask 6) or 1 (mask 7) waves per SIMD, which
  // costs more (+0.41 ms / +3.0 ms) than the slab kernels it removes (0.22 ms / 0.45 ms) -> default 0.
  int pml_fused = -1;                // -1 = default
  // placement of the field arrays: how many alternative sets of allocations the first large run tries (probe_placement)
  int placement_tries = 6;
  int slab_boxes_first = 3;          // FDTD_OPT_SLAB_BOXES_FIRST: the shell's boxes of a CPML slab-rank pair in front of the bulk sweep (1), behind it (0),
                                     // beside it on a stream of their own (2: box_stream), or 2 for slabs of 96 planes and more, else 1 (3, default)
  hipStream_t box_stream = nullptr;  // (made at the first such pair: make_box_stream)
  bool box_stream_tried = false;
  int box_stream_attempts = 0;
  hipEvent_t ev_box = nullptr, ev_box_in = nullptr;      // the boxes done / what st had issued in front of them
  bool placement_done = false;
  float placement_ms[9] = {};      // time of the probe sweeps per candidate (the first is the original)
  int placement_tried = 0, placement_kept = 0;        // candidates timed beyond the original / index of the one kept (0 = original)
  int mem_hints = 1;                 // FDTD_OPT_MEM_HINTS: 1 = non-temporal field stores in the sweep's instantiations without CPML
  int lds_pad = 0;                   // extra dynamic LDS per workgroup of the sweep (bytes): lowers its occupancy — a measuring aid
  int pml_split = -1;                // three launches (interior / y-edge / z-edge tiles): -1 = by grid size, 0 = one launch, 1 = always
  // opt-in (FDTD_OPT_AUTOTUNE): time a few (rows, z-chunk) tile shapes on the first run and keep the
  // best.  Measured (profiles/r01h_autotune.txt): +6 % on a 64-plane slab (3 x 32 instead of 3 x 16),
  // nothing at 512^3 (shapes within noise of each other, so the pick is noise too) and the wrong
  // objective for the pipelined z-slab schedule (it times the whole range) -> off by default.
  int autotune = 0;
  bool tuned = false, user_geometry = false;
  int bnd_planes = 0;                // fused z-slab schedule: planes per boundary chunk (0 = heuristic)
  int rows = 4;
  PmlP* pml_blk[8][2][2] = {};       // device parameter blocks of the in-sweep CPML: [axis mask][psi_h parity][psi_e parity] (E side in place)
  PmlP* pml_blk2[2][2] = {};         // the same for shell2_step_kernel: all axes, both sides read one set and write the other
  PmlP* pml_blk_hole[2][2][2] = {};  // z holes of a shell2 pair: [step of the pair][psi_h parity][psi_e parity] — step one current -> temporary sets, step two temporary -> other sets
  bool pml_blk_hole_ok = false;
  bool pml_blk_ok[8] = {};
  bool pml_blk2_ok = false;
  int pml_parity = 0;
  int pml_e_parity = 0;              // flips when a step pair wrote the E-side psi into the other set (shell2 pairs)
  // RCCL
  ncclComm_t comm = nullptr;
  int rank = 0, n_ranks = 1;
  hipEvent_t ev_h_int = nullptr, ev_h_bnd = nullptr, ev_e_int = nullptr, ev_e_bnd = nullptr;
  // the two streams must really overlap (probe_stream_overlap): 0 = not probed, 1 = verified, -1 = one stream in use
  int stream_overlap = 0, stream_retries = 0;
  bool streams_shared = false;       // comm_stream is an alias of stream (fallback)
  // slab-interleaved two-step schedule (fdtd_run): planes per slab; 0 = off, -1 = default
  int tblock = -1;
  int edge_zchunk = -1;              // z-chunk of the edge launches of a CPML step: -1 = about one wave of workgroups, 0 = as the interior, N = planes
  // Captured step pairs (small grids): a run of steps without monitor records or field-decay checks is replayed as
  // hipGraphs of TWO steps each (set a -> b -> a, psi parity back where it was), one per (field set, psi parity) state
  int use_graph = -1;                // -1 = default (= never: no gain measured, fdtd_run), 0 = never, 1 = whenever possible
  long long* step_dev = nullptr;     // device-side step counter the captured source kernels read
  long long step_dev_value = -1;     // what it holds (host mirror)
  bool step_dev_mode = false;        // launches are being captured: source kernels take step_dev + step_dev_off
  long long step_dev_off = 0;
  long long graph_pairs = 0;
  int mirror_wall[3] = {-1, -1, -1}; // PMC on plus faces: wall index per axis (fdtd_set_mirror_plus), -1 = none
  int graph_status = 0;              // 0 = no capture attempted, 1 = captured, < 0 = -(100 * stage + hipError) of the failed capture
  long long two_step_pairs = 0;
  int tblock_used = 0;
  // two time steps per sweep (fused2_step_kernel): waves per workgroup (0 = off) and planes per chunk
  int twostep_w = -1, twostep_zc = 0;      // -1 / 0: chosen by fused2_shape
  int twostep_w_used = 0, twostep_zc_used = 0;
  long long fused2_pairs = 0;
  // shell pairs: the two-step sweep over the bulk of a CPML-walled grid, its shell (slabs + collar) by two single steps beside
  // it (fdtd_run).  shell_on: -1 = default (on), 0 = off
  int shell_on = -1;
  int strip_zc = 4;                   // planes per workgroup of the x strips (4: 1.199 ms per V2 step, 8: 1.205, 16: 1.228 inside one engine, profiles/r4/r4n)
  int strip_occ = 3;                  // their register budget: workgroups per CU (3 or 4)
  long long shell_pairs = 0;
  // shell2 pairs (round 5): the shell of a CPML-walled grid advanced by shell2_step_kernel — two steps per sweep with psi carried —
  // instead of two single steps through the third field set.  shell2_on: -1 = default (where the cost model likes it), 0 = off, 1 = wherever possible
  int shell2_on = -1;
  int shell2_qw = 0, shell2_ww = 8, shell2_zcw = 0;      // lanes per row of the wide boxes (z / y slabs; 0 = by box), waves per workgroup of the launch, planes per chunk (0 = by box)
  int shell2_ws = 6, shell2_zcs = 0;                     // waves per workgroup of the one-axis launches; x strips: planes per chunk (0 = by box)
  long long shell2_pairs = 0;
  int f2_off_reason = 0;              // why the last fdtd_run took no step pairs (FDTD_F2_OFF_*), 0 = it did / could
  int debug_sync = 0;                 // FDTD_OPT_DEBUG_SYNC: a device-wide synchronisation behind every launch group (dbg_sync) — no two launches ever overlap
  hipEvent_t ev_shell_a = nullptr, ev_shell_b = nullptr;
  hipEvent_t ev_rec = nullptr;        // z-slab ranks: a monitor record on the main stream done (the comm stream's next boundary work waits for it)
  long long seam_deferred_pairs = 0, seam_flushes = 0;      // (of the current fdtd_run: FdtdSeamStats)
  double seam_flush_ms = 0.0;
  std::vector<int64_t> sweep_words;   // distinct (LB, OPT, W) of the two-step sweeps launched since fdtd_create / fdtd_reset (fdtd_get_sweep_words)
  float* seam_buf = nullptr;          // intermediate values on the seams between x tiles, and behind them the compact repair array (deferred seam repair)
  int axis_shift = 0;                 // FDTD_OPT_AXIS_SHIFT: the cyclic renaming the caller applied (device axis a = the caller's axis (a + s) % 3)
  int seam_defer = -1;                // FDTD_OPT_SEAM_DEFER: -1 / 1 = plain sixteen-wave pairs followed by a plain pair leave their repaired seam values in the compact array, 0 = never, 2 = testing aid: at every workgroup size
  bool no_jlo = false;                // $FDTD_NO_JLO at fdtd_create (a debugging aid): no box of a shell pair starts its tile rows on the y-min wall
  bool seam_pending = false;          // the seam columns of the current set (h->f) are stale: their values lie in the repair array
  float* inj_val = nullptr;           // source terms applied between the two steps
  float* cap_val = nullptr;           // samples of the middle step (small time monitors)
  float* dump_buf = nullptr;          // H^{n+1/2} over the boxes of DFT monitors recording at the first step of a pair
  long long dump_cap = 0;
  std::deque<F2Table> f2_tables;      // node tables, one per set of recording monitors met so far (a deque: pointers to its entries stay valid)
  size_t inj_sources = 0;             // point-source lists the tables were built from
  float* src_tab = nullptr;           // [step][node] source terms of every step, formed once (nullptr: per pair)
  long long src_tab_steps = 0, src_tab_nodes = 0;
  bool src_on_seam = false;           // an E-side source node lies next to a seam between x tiles: step n+1's terms go behind the launch
  bool src_h_on_seam = false;         // an H_y / H_z source node in the column left of a seam: no pairs while that list is alive
  long long src_nodes = 0;            // source nodes of all lists
  int f2_dyn_reason = 0;              // the last reason a step of this run could not open a pair because of its sources (FDTD_F2_OFF_*)
  long long src_h_nodes = 0;          // H-side source nodes (need the table of all steps)
  bool src_e_in_damp = false;         // an E-side source node lies inside an absorber layer (its damping factor is not exactly 1)
  bool bloch_pair = false;            // the handle has been one of the two of an fdtd_run_bloch
};

namespace {

int fail(FdtdSolver* h, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return -1;
}

// z-slab handles and Bloch pairs refuse the monitors of `h` that need their whole box on one handle (the error goes to `err`)
int refuse_whole_grid_monitors(FdtdSolver* err, const FdtdSolver* h, const char* who, bool bloch = false) {
  for (const Monitor& m : h->mons)
    if (m.form == MonForm::LatticeDft)
      return fail(err, "%s: lattice DFT monitors%s", who,
                  bloch ? " (fdtd_add_lattice_dft_monitor) are not available with Bloch boundaries (complex fields)" : " are not available on z-slab handles");
  for (const Monitor& m : h->mons)
    if (needs_whole_grid(m))
      return fail(err, "%s: flux-time, sparse field-time and sparse DFT monitors%s", who,
                  bloch ? " (fdtd_add_flux_time_monitor, fdtd_add_field_time_monitor, fdtd_add_field_dft_monitor) are not available with Bloch boundaries (complex fields)"
                        : " are not available on z-slab handles");
  return 0;
}

// ---- the whole-grid node lists of a handle (kListKind): how many of a kind, and list k < n_lists of them --------------------------
size_t n_lists(const FdtdSolver* h, int kind) {
  const size_t n[kListKinds] = {h->aniso.size(), h->modulation.size(), h->conformal.size(), h->nonlinear.size()};
  return n[kind];
}
const ListHead& list_at(const FdtdSolver* h, int kind, size_t k) {
  if (kind == kAniso) return h->aniso[k];
  if (kind == kModulation) return h->modulation[k];
  return kind == kConformal ? (const ListHead&)h->conformal[k] : h->nonlinear[k];
}
// the first kind the handle holds, kListKinds = none: step pairs, tb_pair's slabs and captured graphs are for handles without lists
// (a graph bakes its kernel arguments, and the modulation's phases are arguments that change every step)
int first_list_kind(const FdtdSolver* h) { int k = 0; while (k < kListKinds && !n_lists(h, k)) ++k; return k; }
bool has_lists(const FdtdSolver* h) { return first_list_kind(h) < kListKinds; }
// z-slabs refuse the lists `h` holds (the error goes to `err`).  `early`: asked by fdtd_add_* / fdtd_comm_init — the kinds whose row
// says so; `adding`: the kind fdtd_add_* is about to add to `h`, refused where h is a z-slab handle by its faces or its communicator
int refuse_lists_on_z_slabs(FdtdSolver* err, const FdtdSolver* h, const char* who, bool early = false, int adding = kListKinds) {
  if (adding < kListKinds && !h->comm && h->cfg.bc[4] != FDTD_BC_NEIGHBOR && h->cfg.bc[5] != FDTD_BC_NEIGHBOR) return 0;
  for (int kind = 0; kind < kListKinds; ++kind)
    if ((kind == adding || n_lists(h, kind)) && (kListKind[kind].early || !early))
      return fail(err, "%s: %s are not available on z-slabs", who, kListKind[kind].noun);
  return 0;
}
// the two handles of a Bloch pair: the same lists (component and length, list by list), or none of a kind that Bloch boundaries refuse
int check_bloch_lists(FdtdSolver* hr, const FdtdSolver* hi) {
  for (int kind = 0; kind < kListKinds; ++kind) {
    const char* name = kListKind[kind].bloch_lists;
    if (!name && (n_lists(hr, kind) || n_lists(hi, kind)))
      return fail(hr, "fdtd_run_bloch: %s are not available with Bloch boundaries", kListKind[kind].noun);
    bool same = n_lists(hr, kind) == n_lists(hi, kind);
    for (size_t k = 0; same && k < n_lists(hr, kind); ++k)
      same = list_at(hr, kind, k).comp == list_at(hi, kind, k).comp && list_at(hr, kind, k).n == list_at(hi, kind, k).n;
    if (!same) return fail(hr, "fdtd_run_bloch: the two solvers must carry the same %s", name);
  }
  return 0;
}

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define NCCLCHK(h, call)                                                                  \
  do {                                                                                    \
    ncclResult_t r_ = (call);                                                             \
    if (r_ != ncclSuccess)                                                                \
      return fail(h, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

template <typename T>
int dev_alloc(FdtdSolver* h, T** out, size_t count, bool zero_fill = true) {
  void* p = nullptr;
  size_t bytes = count * sizeof(T);
  if (bytes == 0) bytes = sizeof(T);
  HIPCHK(h, hipMalloc(&p, bytes));
  if (zero_fill) {
    // hipMemset on device memory may return before the fill has run, and it runs on the NULL stream — which the engine's
    // non-blocking streams do not wait for.  Every allocation is handed out filled.
    HIPCHK(h, hipMemset(p, 0, bytes));
    HIPCHK(h, hipStreamSynchronize(nullptr));
  }
  h->bufs.push_back({p, bytes});
  h->stats.device_bytes += (int64_t)bytes;
  *out = reinterpret_cast<T*>(p);
  return 0;
}

template <typename T>
int dev_upload(FdtdSolver* h, T** out, const T* host, size_t count) {
  if (dev_alloc(h, out, count, false)) return -1;
  if (count) HIPCHK(h, hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// The twelve field arrays: one allocation per array.
//
// WHERE they land in device memory decides up to 15 % of the sweep's speed (profiles/r02q_probe_series.jsonl,
// r02t_probe_memory_depth.jsonl: the same kernel on the same box runs 1.174, 1.25 or 1.35 ms per 512^3 step depending
// on the engine's allocations, to +-0.2 % within an engine and with all clocks unchanged; a fresh process's first
// engine normally gets the fast state).  Virtual addresses do not show it, distances between the arrays inside one
// allocation do not change it (r02r), nor does aligning the virtual addresses to the array size — through
// $HSA_MAX_VA_ALIGN or through hipMemAddressReserve + hipMemMap (r02u, r02v: 1.25 ms mapped against 1.17-1.19 ms
// hipMalloc'ed on the same box) — so it is a property of the physical pages, nothing this library controls.
// -DFDTD_PLACEMENT_PROBE compiles the placements those measurements used ($FDTD_FIELD_LAYOUT, scripts/probe_layout.py).
#ifdef FDTD_PLACEMENT_PROBE
// $FDTD_FIELD_LAYOUT, read at every fdtd_create:
//   0  one allocation per array (default)          1  one allocation per field set (six arrays back to back)
//   3  ONE allocation: array c of set q starts at  q * (6 * stride + $FDTD_FIELD_S2) + c * stride  bytes,
//      stride = array bytes + $FDTD_FIELD_S1  (both multiples of 16)
inline long env_long(const char* name, long dflt) {
  const char* e = std::getenv(name);
  return e ? std::atol(e) : dflt;
}
int alloc_field_set(FdtdSolver* h, float** base, size_t fcount, int set) {
  const int mode = (int)env_long("FDTD_FIELD_LAYOUT", 0);
  if (mode == 3 || mode == 4) {
    if (set == 1) return 0;                                   // both sets were placed by the first call
    const size_t s0 = (size_t)env_long("FDTD_FIELD_S0", 0) / 16 * 4;
    const size_t s1 = (size_t)env_long("FDTD_FIELD_S1", 0) / 16 * 4, s2 = (size_t)env_long("FDTD_FIELD_S2", 0) / 16 * 4;
    const size_t stride = fcount + s1;
    float* blk = nullptr;
    if (mode == 4) {                                          // 4: as 3, inside a pool that lives as long as the process
      static float* pool = nullptr;                           //    (the SAME memory for every engine; $FDTD_FIELD_S0 = offset into it)
      const size_t pool_floats = (size_t)env_long("FDTD_FIELD_POOL", 16L << 30) / 4;
      if (!pool) HIPCHK(h, hipMalloc((void**)&pool, pool_floats * 4));
      if (s0 + 12 * stride + s2 > pool_floats) return fail(h, "field pool too small");
      blk = pool + s0;
      HIPCHK(h, hipMemset(blk, 0, (12 * stride + s2) * 4));
    } else if (dev_alloc(h, &blk, 12 * stride + s2)) return -1;
    for (int c = 0; c < 6; ++c) {
      h->fbase[c] = blk + (size_t)c * stride;
      h->fbase2[c] = blk + 6 * stride + s2 + (size_t)c * stride;
    }
    if (env_long("FDTD_DEBUG_ADDR", 0)) std::fprintf(stderr, "field block at %p, stride %zu bytes\n", (void*)blk, stride * 4);
    return 0;
  }
  if (mode == 1) {
    float* blk = nullptr;
    if (dev_alloc(h, &blk, 6 * fcount)) return -1;
    for (int c = 0; c < 6; ++c) base[c] = blk + (size_t)c * fcount;
    return 0;
  }
  // 5: one allocation per array, its size rounded up to a multiple of $FDTD_FIELD_ROUND bytes
  const size_t round = mode == 5 ? (size_t)env_long("FDTD_FIELD_ROUND", 1L << 30) / 4 : 1;
  for (int c = 0; c < 6; ++c) {
    if (dev_alloc(h, &base[c], (fcount + round - 1) / round * round)) return -1;
    if (env_long("FDTD_DEBUG_ADDR", 0)) std::fprintf(stderr, "field set %d array %d at %p\n", set, c, (void*)base[c]);
  }
  return 0;
}

#else
int alloc_field_set(FdtdSolver* h, float** base, size_t fcount, int) {
  for (int c = 0; c < 6; ++c)
    if (dev_alloc(h, &base[c], fcount)) return -1;
  return 0;
}
#endif

constexpr int kBndPlanes = 2;        // boundary chunk of the z-slab schedule, planes per neighbour face (fdtd_run)
constexpr int kPlainZChunk = 8;      // z-chunk of sweeps without in-sweep CPML (launch_fused_range)
constexpr int kTileRun = 8;          // default tile order of the sweep: runs of 8 tiles per XCD (launch_fused_range)
// cost model of shell2 pairs (shell2_why_not): ps per cell and PAIR, measured on MI355X at 512^3 V2 with each launch alone on
// the machine (profiles/r5/r5d, r5e): the clipped bulk sweep 12.9 (with materials; 11.3 without), a cell of a wide box 27, a
// strip cell 41 (the boxes as one launch: 0.69 ms for 21.3 M cells, half of it the strips); the two streams overlap to 0.93 of
// the sum; a single step costs 10.1 ps per cell.  V2: predicted 0.74 of two single steps, measured 0.76; BASELINE config 3 laid
// out with x = 224: predicted 0.83, measured 0.86.
constexpr double kShell2BulkPs = 11.3, kShell2BulkMatPs = 12.9, kShell2WidePs = 27.0, kShell2StripPs = 41.0, kShell2Overlap = 0.93;

inline unsigned nblk(long long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// planes [k0, k1) touched by a list of linear cell indices (empty list: k0 == k1 == 0)
inline void plane_range(const uint32_t* cell, long long n, long long sxy, int* k0, int* k1) {
  *k0 = *k1 = 0;
  if (n <= 0) return;
  uint32_t lo = cell[0], hi = cell[0];
  for (long long i = 1; i < n; ++i) { lo = std::min(lo, cell[i]); hi = std::max(hi, cell[i]); }
  *k0 = (int)(lo / (uint64_t)sxy);
  *k1 = (int)(hi / (uint64_t)sxy) + 1;
}
inline bool planes_meet(int k0, int k1, int kbeg, int kend) { return k0 < kend && kbeg < k1; }

// Every non-empty side of every source list, in the order launch_sources adds them at a step: TFSF boxes first, then point lists, in
// the order they were added; within each the E side before the H side.  fn(side, is the H side) with a TfsfList& or a PointSide&:
// both name n, cell, comp, soff and layer alike.  The paged source terms take their layers in this order (spg_setup), and spg_fill
// and launch_sources walk one side at a time in the same order of lists.
template <typename Solver, typename Fn>
void for_each_source_side(Solver* h, Fn fn) {
  for (auto& t : h->tfsf) {
    if (t.e.n) fn(t.e, false);
    if (t.h.n) fn(t.h, true);
  }
  for (auto& s : h->psrc) {
    if (s.e.n) fn(s.e, false);
    if (s.h.n) fn(s.h, true);
  }
}
// a point list's E side injects at step n: something is still to be added to E behind a sweep that did not add it itself
bool e_sources_due(const FdtdSolver* h, long long n) {
  for (const PointSrc& s : h->psrc) if (s.e_due(n)) return true;
  return false;
}

// Lays out the segment map of a paging: `mark(M.dev)` launches disp_mark_kernel on h->stream for every list; the marked segments are
// numbered 0 .. n_blocks - 1 in map order, the others become -1, on the host and on the device.  0 = built; 1 = the caller gives up
// (no memory, no marked segment, or more floats in [n_blocks][3][256] than a 32-bit slot addresses); -1 = a HIP error.
template <typename Mark>
int seg_map_build(FdtdSolver* h, SegMap& M, Mark mark) {
  const size_t nseg = (size_t)h->g.nz * h->g.ny * ((h->g.nx + 255) / 256);
  hipStream_t st = h->stream;
  if (dev_alloc(h, &M.dev, nseg)) return 1;
  mark(M.dev);
  M.host.assign(nseg, 0);
  HIPCHK(h, hipMemcpyAsync(M.host.data(), M.dev, nseg * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  long long nb = 0;
  for (size_t q = 0; q < nseg; ++q) M.host[q] = M.host[q] ? (int)nb++ : -1;
  if (nb == 0 || nb * 3 * 256 >= (1LL << 32)) return 1;
  HIPCHK(h, hipMemcpyAsync(M.dev, M.host.data(), nseg * sizeof(int), hipMemcpyHostToDevice, st));
  M.n_blocks = (int)nb;
  return 0;
}
// the empty bounding box {lo, hi} per axis that the slot kernels of a paging (disp_qoff_kernel, src_soff_kernel) widen
int box_seed_upload(FdtdSolver* h, int** box) {
  const int big = 1 << 30;
  const int box0[6] = {big, -1, big, -1, big, -1};
  return dev_upload(h, box, box0, 6);
}

long long plane_cells(const FdtdSolver* h) { return (long long)h->cfg.nx * h->cfg.ny; }
long long n_cells(const FdtdSolver* h) { return plane_cells(h) * h->cfg.nz; }

float* field_ptr(FdtdSolver* h, int comp) {
  switch (comp) {
    case 0: return h->f.ex; case 1: return h->f.ey; case 2: return h->f.ez;
    case 3: return h->f.hx; case 4: return h->f.hy; default: return h->f.hz;
  }
}

StepP step_params(const FdtdSolver* h) {
  StepP s;
  s.ipx = h->ip[0]; s.ipy = h->ip[1]; s.ipz = h->ip[2];
  s.idx = h->idl[0]; s.idy = h->idl[1]; s.idz = h->idl[2];
  return s;
}

MatP mat_params(const FdtdSolver* h) {
  MatP m;
  m.m4 = h->mat4;
  m.m4b = h->mat4b;
  m.roww = h->roww;
  m.lut = h->lut; m.n_media = h->n_media; m.ca1 = h->ca1; m.cb1 = h->cb1;
  return m;
}

// ---- timing of the main kernels -----------------------------------------------------------
// FDTD_OPT_DEBUG_SYNC: everything issued so far — on either stream — has finished before the next launch group goes out.  Called at
// the head of every launch helper and around every sweep launch: with it no two launches of a run ever overlap, so a result that
// differs from the normal run's points at a missing cross-stream edge (tests/test_gpu_parity.py).
inline void dbg_sync(const FdtdSolver* h) { if (h->debug_sync) (void)hipDeviceSynchronize(); }

void time_begin(FdtdSolver* h, int kind, hipStream_t st) {
  dbg_sync(h);
  if (!(h->cfg.flags & FDTD_FLAG_TIME_KERNELS)) return;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  hipEventRecord(a, st);
  h->kev.push_back(a);
  h->kev.push_back(b);
  h->kev_kind.push_back(kind);
}
void time_end(FdtdSolver* h, hipStream_t st) {
  dbg_sync(h);
  if (!(h->cfg.flags & FDTD_FLAG_TIME_KERNELS)) return;
  hipEventRecord(h->kev.back(), st);
}

// ---- launches -------------------------------------------------------------------------------
void launch_h_main(FdtdSolver* h, int kbeg, int kend, hipStream_t st) {
  if (kend <= kbeg) return;
  const GridP& g = h->g;
  const bool vec = (g.nx % 4 == 0) && h->cfg.variant != FDTD_VARIANT_SIMPLE;
  const int V = vec ? 4 : 1;
  const int zc = (h->cfg.variant == FDTD_VARIANT_SIMPLE) ? 1 : h->zchunk;
  const int rows = h->rows;                             // <= 8: __launch_bounds__(512)
  dim3 block(64, rows, 1);
  dim3 grid((g.nx + 64 * V - 1) / (64 * V), (g.ny + rows - 1) / rows, (kend - kbeg + zc - 1) / zc);
  time_begin(h, 0, st);
  if (vec)
    hipLaunchKernelGGL((h_update_kernel<4>), grid, block, 0, st, g, h->f, step_params(h), kbeg, kend, zc);
  else
    hipLaunchKernelGGL((h_update_kernel<1>), grid, block, 0, st, g, h->f, step_params(h), kbeg, kend, zc);
  time_end(h, st);
}

void launch_e_main(FdtdSolver* h, int kbeg, int kend, hipStream_t st) {
  if (kend <= kbeg) return;
  const GridP& g = h->g;
  const bool vec = (g.nx % 4 == 0) && h->cfg.variant != FDTD_VARIANT_SIMPLE;
  const int V = vec ? 4 : 1;
  const int zc = (h->cfg.variant == FDTD_VARIANT_SIMPLE) ? 1 : h->zchunk;
  const bool has_mat = h->mat4 != nullptr;
  const int rows = h->rows;                             // <= 8: __launch_bounds__(512)
  dim3 block(64, rows, 1);
  dim3 grid((g.nx + 64 * V - 1) / (64 * V), (g.ny + rows - 1) / rows, (kend - kbeg + zc - 1) / zc);
  MatP m = mat_params(h);
  StepP s = step_params(h);
  time_begin(h, 1, st);
  if (vec && has_mat)
    hipLaunchKernelGGL((e_update_kernel<4, true>), grid, block, 0, st, g, h->f, s, m, kbeg, kend, zc);
  else if (vec)
    hipLaunchKernelGGL((e_update_kernel<4, false>), grid, block, 0, st, g, h->f, s, m, kbeg, kend, zc);
  else if (has_mat)
    hipLaunchKernelGGL((e_update_kernel<1, true>), grid, block, 0, st, g, h->f, s, m, kbeg, kend, zc);
  else
    hipLaunchKernelGGL((e_update_kernel<1, false>), grid, block, 0, st, g, h->f, s, m, kbeg, kend, zc);
  time_end(h, st);
}

// fused E+H sweep over the planes [kbeg, kend): reads the current set, writes the other one
int ensure_second_set(FdtdSolver* h) {
  const GridP& g = h->g;
  if (h->f2.ex) return 0;
  const size_t fcount = (size_t)g.sxy * (g.nz + 2);
  if (!h->fbase2[0] && alloc_field_set(h, h->fbase2, fcount, 1)) return -1;
  h->f2.ex = h->fbase2[0] + g.sxy; h->f2.ey = h->fbase2[1] + g.sxy; h->f2.ez = h->fbase2[2] + g.sxy;
  h->f2.hx = h->fbase2[3] + g.sxy; h->f2.hy = h->fbase2[4] + g.sxy; h->f2.hz = h->fbase2[5] + g.sxy;
  return 0;
}

bool any_pml(const FdtdSolver* h) {
  for (int a = 0; a < 3; ++a) if (h->pml[a].n_lo + h->pml[a].n_hi > 0) return true;
  return false;
}

// ---- device parameter blocks of the in-sweep CPML (PmlP), built on first use ----------------------------------------------------
// the lazily allocated psi sets named in `which` (bits 1 << PmlAxisDev::kH2 ...) of every axis with members; *e2_fresh: the second
// E-side set was allocated by this call
int ensure_psi_sets(FdtdSolver* h, int which, bool* e2_fresh = nullptr) {
  for (int a = 0; a < 3; ++a) {
    PmlAxisDev& P = h->pml[a];
    if (P.ns == 0) continue;
    for (int q = 0; q < 2; ++q)
      for (int s = PmlAxisDev::kH2; s < PmlAxisDev::kSets; ++s) {
        if (!((which >> s) & 1) || P.set(s)[q]) continue;
        if (dev_alloc(h, &P.set(s)[q], P.set_count(s))) return -1;
        if (s == PmlAxisDev::kE2 && e2_fresh) *e2_fresh = true;
      }
  }
  return 0;
}
// every parameter block is rebuilt on its next use
void invalidate_pml_blocks(FdtdSolver* h) {
  for (bool& ok : h->pml_blk_ok) ok = false;
  h->pml_blk2_ok = false; h->pml_blk_hole_ok = false;
}

// which sets of an axis a block reads and writes.  "Current" is what the host calls psi_h / psi_e at the time of the launch,
// "other" what it calls psi_h2 / psi_e2.
enum PsiRoute {
  kPsiEInPlace,     // sweeps of single steps: the H side reads the current set and writes the other one, the E side stays in place
  kPsiPingPong,     // shell2_step_kernel: both sides read the current sets and write the other ones
  kPsiToTemp,       // z hole of a shell2 pair, step one: both sides current -> temporary sets
  kPsiFromTemp,     // z hole, step two: both sides temporary -> other sets
};
// flip_h / flip_e: the block is for the parity opposite to the one the host's names have now (upload_pml_block)
void fill_pml_axis(const FdtdSolver* h, int a, bool in, bool flip_h, bool flip_e, PsiRoute route, PmlAxisP& A) {
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  const PmlAxisDev& P = h->pml[a];
  A.ce4 = P.ce4; A.ch4 = P.ch4;
  A.kv_e = P.kv_e; A.b_e = P.b_e; A.c_e = P.c_e;
  A.kv_h = P.kv_h; A.b_h = P.b_h; A.c_h = P.c_h;
  float *rd_e[2], *wr_e[2], *rd_h[2], *wr_h[2];
  for (int q = 0; q < 2; ++q) {
    // (without a second E-side set both parities name the one set there is)
    float* const e_cur = flip_e && P.psi_e2[q] ? P.psi_e2[q] : P.psi_e[q];
    float* const e_oth = flip_e || !P.psi_e2[q] ? P.psi_e[q] : P.psi_e2[q];
    float* const h_cur = flip_h ? P.psi_h2[q] : P.psi_h[q];
    float* const h_oth = flip_h ? P.psi_h[q] : P.psi_h2[q];
    rd_e[q] = route == kPsiFromTemp ? P.psi_et[q] : e_cur;
    rd_h[q] = route == kPsiFromTemp ? P.psi_ht[q] : h_cur;
    wr_e[q] = route == kPsiEInPlace ? e_cur : (route == kPsiToTemp ? P.psi_et[q] : e_oth);
    wr_h[q] = route == kPsiToTemp ? P.psi_ht[q] : h_oth;
  }
  A.pe0 = rd_e[0]; A.pe1 = rd_e[1]; A.pe0n = wr_e[0]; A.pe1n = wr_e[1];
  A.ph0 = rd_h[0]; A.ph1 = rd_h[1]; A.ph0n = wr_h[0]; A.ph1n = wr_h[1];
  // an axis without CPML, or one whose recursions stay in the slab kernels, has no members
  A.lo = in ? P.lo : 0; A.hi0 = in ? P.hi0 : N[a]; A.ns = P.ns; A.n = N[a];
}
// One block into one slot: the axes of `mask` with their recursions inside the kernel, for H-side parity `par` and E-side parity `ep`.
// The two sets of an axis keep their identity: `psi_h` / `psi_h2` (`psi_e` / `psi_e2`) swap NAMES on the host after every sweep that
// carried the axis (swap_psi_h: the axes of its mask only — launch_pml reads the un-swapped names of the others) or shell2 pair
// (swap_psi_e), and pml_parity / pml_e_parity count the swaps.  A block is indexed by the parities at the time of its launch, but
// filled from the names as they are NOW: block [par][ep] must read what the host will call psi_h (psi_e) when pml_parity == par
// (pml_e_parity == ep) — today's psi_h2 (psi_e2) when that parity differs from today's.
int upload_pml_block(FdtdSolver* h, PmlP** slot, int mask, int par, int ep, PsiRoute route) {
  PmlP pm{};
  for (int a = 0; a < 3; ++a)
    fill_pml_axis(h, a, h->pml[a].ns > 0 && ((mask >> a) & 1), par != h->pml_parity, ep != h->pml_e_parity, route, pm.ax[a]);
  if (!*slot && dev_alloc(h, slot, 1, false)) return -1;
  if (hipMemcpy(*slot, &pm, sizeof(PmlP), hipMemcpyHostToDevice) != hipSuccess)
    return fail(h, "upload of the CPML parameter block failed");
  return 0;
}
// the blocks of the sweeps of single steps: [axes inside the sweep][par][ep]
int ensure_pml_blocks(FdtdSolver* h, int mask) {
  if (h->pml_blk_ok[mask]) return 0;
  if (ensure_psi_sets(h, 1 << PmlAxisDev::kH2)) return -1;
  for (int par = 0; par < 2; ++par)
    for (int ep = 0; ep < 2; ++ep)
      if (upload_pml_block(h, &h->pml_blk[mask][par][ep], mask, par, ep, kPsiEInPlace)) return -1;
  h->pml_blk_ok[mask] = true;
  return 0;
}
// the blocks of shell2_step_kernel: all axes with layers.  The second E-side set is allocated here; the in-place blocks name it for
// the other parity, so a fresh one sends them to be rebuilt (no hole block can be valid without it)
int ensure_pml_blocks2(FdtdSolver* h) {
  if (h->pml_blk2_ok) return 0;
  bool fresh = false;
  if (ensure_psi_sets(h, 1 << PmlAxisDev::kH2 | 1 << PmlAxisDev::kE2, &fresh)) return -1;
  if (fresh) invalidate_pml_blocks(h);
  for (int par = 0; par < 2; ++par)
    for (int ep = 0; ep < 2; ++ep)
      if (upload_pml_block(h, &h->pml_blk2[par][ep], 7, par, ep, kPsiPingPong)) return -1;
  h->pml_blk2_ok = true;
  return 0;
}

// The blocks of the z holes of a shell2 pair (planes that take two single steps beside the boxes: a mode plane, the injection plane
// of a plane wave).  The boxes around a hole re-read the OLD psi of its planes (chunk prologues, the plane above a chunk) while the
// hole's first step runs, so that step writes TEMPORARY sets on both sides and the second one reads them and writes the sets the
// boxes write — after the pair every cell's psi sits in the same (new) sets.
int ensure_pml_blocks_hole(FdtdSolver* h) {
  if (h->pml_blk_hole_ok) return 0;
  if (ensure_pml_blocks2(h)) return -1;
  if (ensure_psi_sets(h, 1 << PmlAxisDev::kHt | 1 << PmlAxisDev::kEt)) return -1;
  for (int step = 0; step < 2; ++step)
    for (int par = 0; par < 2; ++par)
      for (int ep = 0; ep < 2; ++ep)
        if (upload_pml_block(h, &h->pml_blk_hole[step][par][ep], 7, par, ep, step == 0 ? kPsiToTemp : kPsiFromTemp)) return -1;
  h->pml_blk_hole_ok = true;
  return 0;
}

// axes whose CPML recursions can run inside the sweep
int pml_in_sweep_mask(const FdtdSolver* h) {
  int mask = 0;
  for (int a = 0; a < 3; ++a) if (h->pml[a].ns > 0) mask |= 1 << a;
  return mask;
}

// after a sweep that carried CPML recursions: the write set becomes the read set
void swap_psi_h(FdtdSolver* h, int pml_inside) {
  if (!pml_inside) return;
  for (int a = 0; a < 3; ++a) {
    PmlAxisDev& P = h->pml[a];
    if (P.ns == 0 || !((pml_inside >> a) & 1)) continue;
    std::swap(P.psi_h[0], P.psi_h2[0]);
    std::swap(P.psi_h[1], P.psi_h2[1]);
  }
  h->pml_parity ^= 1;
}

// after a shell2 pair: the E side too
void swap_psi_e(FdtdSolver* h) {
  for (int a = 0; a < 3; ++a) {
    PmlAxisDev& P = h->pml[a];
    if (P.ns == 0 || !P.psi_e2[0]) continue;
    std::swap(P.psi_e[0], P.psi_e2[0]);
    std::swap(P.psi_e[1], P.psi_e2[1]);
  }
  h->pml_e_parity ^= 1;
}

// Tile rows: all of them (ty_n < 0) or  [0, ty_a) + [ty_a + ty_gap, ty_a + ty_gap + (ty_n - ty_a)).
// pml_inside: axes whose CPML recursions this launch carries (its tiles must not touch members of other
// in-sweep axes): 0 -> plain instantiation, 1 -> the x-only one, anything else -> the all-axes one.
// A shell step (ShellSets) names its own read / write sets and psi parity, and the rows [ex_j0, ex_j1) its launch leaves alone.
struct ShellSets { FieldP src, dst; int parity; int ex_j0, ex_j1; const PmlP* pm = nullptr; };     // pm: a parameter block of the caller's (z holes of a shell2 pair)
// One launch of the sweep: planes [k0, k1) and [k2_0, k2_1), `pml` = pml_inside; call sites name the fields they set.
struct FusedRange { int k0, k1; int pml = 0; int k2_0 = 0, k2_1 = 0; int ty_n = -1, ty_a = 0, ty_gap = 0; bool edge = false; const ShellSets* sh = nullptr; };
// launches <fused_word(L)>, exactly, or returns false with nothing launched: the list of fdtd_fused.hpp as case labels — this line
// instantiates the 42 kernels of the single-step sweep
FDTD_F1_LAUNCHER(launch_fused_step, FDTD_F1_LIST)
int launch_fused_range(FdtdSolver* h, hipStream_t st, const FusedRange& r) {
  int kbeg = r.k0, kend = r.k1, k2beg = r.k2_0, k2end = r.k2_1, ty_n = r.ty_n, ty_a = r.ty_a, ty_gap = r.ty_gap;
  const int pml_inside = r.pml;
  const bool edge = r.edge;
  const ShellSets* sh = r.sh;
  if (kend <= kbeg) {                 // first plane range empty: the second one takes its place
    if (k2end <= k2beg) return 0;
    kbeg = k2beg; kend = k2end; k2beg = k2end = 0;
  }
  if (ty_n == 0) return 0;
  const GridP& g = h->g;
  const int R = h->rows_f;
  // the word of the launch (fdtd_fused.hpp): material form, launch bound (the register budget follows the workgroup size), CPML form, hint
  const int matf = h->mat4 ? (h->mat4b ? 2 : 1) : 0;
  const FusedWord w = fused_word(matf, 64 * (R + 1), h->fused_lb, pml_inside, h->mem_hints);
  const auto no_sweep = [&] {
    return fail(h, "launch_fused_range: no instantiation of the sweep for the word (material form %d, launch bound %d, CPML form %d, hint %d), %d threads",
                w.matf, w.lb, w.pml, w.hint, 64 * (R + 1));
  };
  if (!fused_instantiated(w)) return no_sweep();       // (in front of everything that changes the handle's state)
  if (ensure_second_set(h)) return -1;
  if (pml_inside && ensure_pml_blocks(h, pml_inside)) return -1;
  // z-chunk: 16 planes per workgroup when CPML runs inside the sweep, 8 when not — measured inside engines: 8 is
  // 0 ... 1.5 % faster on the 512^3 plain / materials sweeps and 2 % slower on the CPML-carrying step (profiles/
  // r03f), 2.5 ... 4.5 % faster on the 64- and 128-plane slabs a rank of an 8- / 4-GPU run holds (r03n).  A shape set
  // through fdtd_set_option or found by the tile-shape probe is kept.
  int zc = (h->user_geometry || h->tuned || pml_inside) ? h->zchunk_f : std::min(h->zchunk_f, kPlainZChunk);
  if (ty_gap == 0 && !edge) h->last_zc = zc;            // (the interior launch of a step, not its edge launches)
  // Edge launches of a CPML step (the few tiles that meet a y / z slab, all-axes instantiation): on a thin z-slab they are a
  // handful of workgroups marching the whole slab one plane at a time — 80 workgroups x 16 planes took 83 us alone on the
  // machine, in front of the 179 us interior launch of the same stream (profiles/r3e: 64-plane slab, CPML on x and y).
  // Shorter chunks turn them into about one wave of workgroups (the prologue plane per chunk is cheap on 6 % of the tiles).
  // On ONE GPU the edge launches run on the second stream beside the interior launch and are off the critical path: there
  // the long chunks stay (512^3 V2 inside one engine, profiles/r3f: 16 planes 1.367 ms, 8 planes 1.377, 4 planes 1.394).
  if (edge && sh && h->edge_zchunk < 0) zc = std::min(zc, 8);       // shell steps (beside the bulk sweep of a shell pair): profiles/r4d
  else if (edge && (h->edge_zchunk > 0 || (h->edge_zchunk < 0 && h->comm != nullptr))) {
    const int nby_e = ty_n < 0 ? (g.ny + R - 1) / R : ty_n;
    const long long wg_planes = (long long)((g.nx + 255) / 256) * nby_e * ((kend - kbeg) + std::max(0, k2end - k2beg));
    const int want = h->edge_zchunk > 0 ? h->edge_zchunk : (int)std::max(2LL, std::min((long long)zc, wg_planes / 1024));
    zc = std::min(zc, want);
  }
  const int nby_all = (g.ny + R - 1) / R;
  if (ty_n < 0) { ty_n = nby_all; ty_a = nby_all; ty_gap = 0; }
  const int nbx = (g.nx + 255) / 256, nby = ty_n, nbz1 = (kend - kbeg + zc - 1) / zc;
  const int nbz = nbz1 + (k2end > k2beg ? (k2end - k2beg + zc - 1) / zc : 0);
  const int total = nbx * nby * nbz;
  // Tile order (kernel: launch argument xcd_remap).  Default: runs of 8 consecutive tiles (y-neighbours) per XCD, the
  // runs round-robin over the XCDs.  Measured INSIDE engines held side by side (the only comparison free of the
  // placement effect; profiles/r03d_probe_grouped_tile_order.jsonl, r03e_*): faster than the plain order in every
  // engine (plain sweep -1.4 ... -5 %, materials -1.2 ... -3.8 %, CPML-carrying three-launch step -1.3 ... -2.3 %)
  // and than the contiguous one-eighth-per-XCD split of round 1 (-1.8 ... -9 %), which moves fewer bytes (7.1 vs
  // 8.6 GB per 512^3 sweep in the plain order) but has the eight XCDs stream eight distant regions of every array.
  // Runs of 6 ... 32 tiles are within 0.5 % of each other.
  const int remap = h->xcd_remap < 0 ? kTileRun : h->xcd_remap;
  const int pmc = h->cfg.bc[4] == FDTD_BC_PMC;
  time_begin(h, sh ? 3 : 2, st);
  const PmlP* pm = pml_inside ? ((sh && sh->pm) ? sh->pm : h->pml_blk[pml_inside][sh ? sh->parity : h->pml_parity][h->pml_e_parity]) : nullptr;
  const bool launched = launch_fused_step(FusedLaunch{
      st, remap ? ((total + 7) / 8) * 8 : total, R + 1, matf, h->fused_lb, pml_inside, h->mem_hints, (size_t)h->lds_pad,
      g, sh ? sh->src : h->f, sh ? sh->dst : h->f2, step_params(h), mat_params(h), kbeg, kend, zc, pmc, nbx, nby, nbz, remap, pm,
      nbz1, k2beg, k2end, ty_a, ty_gap, sh ? sh->ex_j0 : 0, sh ? sh->ex_j1 : 0});
  time_end(h, st);
  if (!launched) return no_sweep();       // (the launcher's case labels and fused_instantiated expand the same list)
  return 0;
}

void swap_sets(FdtdSolver* h) {
  std::swap(h->f, h->f2);
  for (int c = 0; c < 6; ++c) std::swap(h->fbase[c], h->fbase2[c]);
}

int launch_fused(FdtdSolver* h, hipStream_t st, int pml_inside) {
  if (launch_fused_range(h, st, {.k0 = 0, .k1 = h->g.nz, .pml = pml_inside})) return -1;
  swap_sets(h);
  swap_psi_h(h, pml_inside);
  return 0;
}

// ---- two time steps per sweep (fdtd_kernels2.hpp) --------------------------------------------------------------------
// What fused2_step_kernel covers: the curl stencil with non-dispersive media (uniform, or packed medium words + (Ca, Cb)
// table: dielectrics, conductors, PEC bodies) inside six PEC walls on one GPU, driven by point sources (electric and magnetic), recorded by
// small time monitors; the min faces may be PMC walls; absorber layers (applied in registers).  Anything else (CPML, ADE,
// TFSF, periodic / Bloch faces, PMC on max faces, z-slabs) takes single steps.
// Tile shape of the two-step sweep: waves per workgroup W (W - 3 rows of a tile are written) and planes per chunk zc (a
// chunk runs zc + 2 plane iterations).  Asked for through FDTD_OPT_TWOSTEP, or (default) the cheapest of W = 8 / 16 x
// zc = 8 ... 64 under a two-parameter model fitted to profiles/r3r_two_step_small.jsonl, r3r_two_step_shapes512.jsonl and
// r3s_two_step_auto_shapes.jsonl:
//   time ~ rounds of workgroups x (zc + 2) x t_W,   16 waves: one workgroup per CU, t = 8.2 us per plane iteration;
//                                                    8 waves: two per CU, t = 6.0 us
// (rounds counted whole while there are fewer than four: the tail of a short launch is real).  It picks the measured best
// or a shape within 3 % of it at 128^3 ... 512^3: 8 waves on grids up to 256^3 (416 workgroups of 5 rows fill the 512 slots
// at once: 195 Gcells/s against 140 with 16 waves), 16 waves from 320^3 on.  Grids below 2^20 cells keep single steps.
// `box` (a clipped launch: the bulk of a shell pair or of a z-slab rank's pair): rows and planes of the box, and chunks of
// EQUAL length — on the 60 bulk planes of a 64-plane slab rank the fixed lengths leave one round of 412 8-wave workgroups
// marching 32 iterations (237 us) where 240 16-wave ones march 22 (profiles/r4e).
bool fused2_shape(const FdtdSolver* h, int* W, int* zc, const ClipP* box = nullptr) {
  const GridP& g = h->g;
  const int nbx = (g.nx + 255) / 256;
  if (h->twostep_w > 0 && h->twostep_zc > 0) { *W = h->twostep_w; *zc = std::max(2, std::min(h->twostep_zc, g.nz)); return true; }
  if (h->twostep_w <= 0 && (long long)g.nx * g.ny * g.nz < (1LL << 20)) return false;
  double best = 0.0;
  bool found = false;
  if (box) {
    const int nyb = box->j1 - box->j0, nzb = box->k1 - box->k0;
    for (int w : {16, 8}) {
      if (h->twostep_w > 0 && w != h->twostep_w) {
        if (w == 16) w = h->twostep_w; else continue;
      }
      const int R = w - 3, nby = (nyb + R - 1) / R;
      // Round 6 (profiles/r6/r6w_slab_shapes.jsonl: 512 x 512 slabs of 64 / 128 / 256 planes, forced shapes against the model of
      // rounds 3 - 5, which took 8 waves everywhere): per plane iteration a 16-wave workgroup takes 6.6 us + 2.1 us x (how full the
      // launch's rounds of 256 are) — 8.6 when two rounds are nearly full — and 1.4 x that when the launch is ONE round (every
      // plane's latency exposed: 16 x 20 on the 60 planes of a 64-plane slab 278 us per pair); an 8-wave one 7.2 us (two per CU), not
      // the 6.0 fitted to 256^3 grids; a chunk costs its two extra iterations and ~1.5 more (prologue, ramp).  64 planes: 8 x 30
      // 253 us per pair, 16 x 10 234; 128 planes: 8 x 18 461, 16 x 21 400; 256 planes: 8 x 23 815, 16 x 42 752 — the shapes this picks.
      // (a rank that carries CPML runs the shell's boxes and the cut planes' single steps beside the bulk: a single round is not left
      //  alone on the machine — 64 planes with layers on x / y: 16 x 20 0.180 ms per step, 16 x 10 0.197, 8 x 30 0.256; 128 planes: 16 x 21
      //  0.338, 16 x 42 0.343, r6x_slab_shapes_pml2)
      const double one_round = any_pml(h) ? 1.1 : 1.4;
      const double slots = w <= 8 ? 512.0 : 256.0;
      for (int nch = 1; nch <= std::max(1, nzb / 4); ++nch) {
        const int c = (nzb + nch - 1) / nch;
        if (c > 64) continue;
        const double wg = (double)nbx * nby * ((nzb + c - 1) / c);
        double rounds = wg / slots;
        if (rounds < 4.0) rounds = std::ceil(rounds);
        const double fill = wg / (std::ceil(wg / slots) * slots);
        const double t8 = 7.2 + (h->mat4 ? 1.6 : 0.0), t16 = (6.6 + 2.1 * fill) * (rounds <= 1.0 ? one_round : 1.0) + (h->mat4 ? 1.2 : 0.0);
        const double t = w <= 8 ? t8 : (w >= 16 ? t16 : t8 + (t16 - t8) * (w - 8) / 8.0);
        const double cost = rounds * (c + 3.5) * t;
        if (!found || cost < best * 0.999) { best = cost; *W = w; *zc = c; found = true; }
      }
    }
    *zc = std::max(2, std::min(*zc, nzb));
    return found;
  }
  for (int w : {16, 8}) {
    if (h->twostep_w > 0 && w != h->twostep_w) {
      if (w == 16) w = h->twostep_w; else continue;        // a requested W: only the chunk length is chosen
    }
    const int R = w - 3, nby = (g.ny + R - 1) / R;
    // (with materials the instantiation sits at 128 VGPRs with 4 spills and looks coefficients up: 512^3 V1 0.800 ms per step
    //  with 16 waves, 0.882 with 8 against 1.136 for single sweeps, profiles/r3zx)
    // (absorber layers damped in registers, 512^3 with 40 layers: 0.959 / 1.014 ms per step with 16 / 8 waves, 1.104 / 1.185 with
    //  materials too, profiles/r3zs)
    // (round 6: 6.0 us per plane iteration of an 8-wave workgroup holds while the launch is ONE round — 256^3: 416 workgroups on 512
    //  slots — launches of several rounds measure 7.2 - 7.7 (slab ranks, r6w) and 320^3 / 384^3 prefer 16 waves: 8 x 16 127 against
    //  16 x 64 136 Gcells/s, 8 x 24 154 against 16 x 48 157, profiles/r6/r6sh_v0_shapes.jsonl)
    const double t16 = 8.2 + (h->mat4 ? 1.2 : 0.0) + (h->has_damp ? 3.0 : 0.0) + (h->mat4 && h->has_damp ? 0.5 : 0.0);
    const double slots = w <= 8 ? 512.0 : 256.0;
    for (int c : {64, 48, 32, 24, 16, 12, 8}) {
      if (c > std::max(8, g.nz)) continue;
      const double wg = (double)nbx * nby * ((g.nz + c - 1) / c);
      double rounds = wg / slots;
      if (rounds < 4.0) rounds = std::ceil(rounds);
      const double t8 = (rounds <= 1.0 ? 6.0 : 6.8) + (h->mat4 ? 1.6 : 0.0) + (h->has_damp ? 2.7 : 0.0);
      const double t = w <= 8 ? t8 : (w >= 16 ? t16 : t8 + (t16 - t8) * (w - 8) / 8.0);
      const double cost = rounds * (c + 2) * t;
      // (16 waves are tried first; 8 waves must be 8 % cheaper under the model to replace them: inside its error the measured
      //  times are equal or favour 16 waves — 512^3 0.703 / 0.709 ms, 1024^3 16 x 64 best, profiles/r3w, r3zw)
      // (on grids below 2^26 cells the model's margin is real: 256^3 8 x 32 183-195 Gcells/s against 168-175 with 16 waves)
      const bool big = (long long)g.nx * g.ny * g.nz >= (1LL << 26);
      if (!found || cost < best * (big && w <= 8 && *W > 8 ? 0.92 : 0.999)) { best = cost; *W = w; *zc = c; found = true; }
    }
  }
  *zc = std::max(2, std::min(*zc, g.nz));
  return found;
}

// Why a run takes no step pairs (FDTD_F2_OFF_*, include/fdtd_hip.h); 0 = nothing in the problem keeps the two-step sweep
// from it.  CPML is not a reason here: the caller then asks shell_eligible.
int fused2_why_not(const FdtdSolver* h, bool slab_rank = false, bool shell = false) {
  if (h->twostep_w == 0) return FDTD_F2_OFF_DISABLED;
  // (first of the problem's own reasons: no two-step sweep, strip or shell box reads the second word per cell, and every pair
  //  form asks here — shell_why_not, shell2_why_not, the z-slab pairs — before it launches anything)
  if (h->mat4b) return FDTD_F2_OFF_WIDE_TABLE;
  { int W, zc; if (!fused2_shape(h, &W, &zc)) return FDTD_F2_OFF_TOO_SMALL; }
  if (h->comm && !slab_rank) return FDTD_F2_OFF_COMM;
  // (a shell pair: the planes that hold dispersive cells are a z hole of the bulk; round 6: the pair advances them itself once
  //  their memory terms are paged, disp_setup)
  if (!h->ade.empty() && !shell && h->disp.state != 1) return FDTD_F2_OFF_ADE;
  if (has_lists(h)) return kListKind[first_list_kind(h)].f2_off;   // whole-grid lists: their kernels go around every single step
  // (sources are judged step by step, fused2_sources_why_not: a TFSF box or a mode plane keeps single steps only while it injects)
  // PEC walls; the min faces may be PMC (the symmetry planes of a half / quarter / eighth domain)
  // (a z-slab rank: a neighbour face is no wall — the sweep stays two planes clear of it, fdtd_run)
  // (a shell pair: a periodic y / z face has the two rows / planes next to it in the shell, periodic x wraps inside the sweep)
  for (int f = 0; f < 6; ++f)
    if (h->cfg.bc[f] != FDTD_BC_PEC && !((f & 1) == 0 && h->cfg.bc[f] == FDTD_BC_PMC) &&
        !(slab_rank && f >= 4 && h->cfg.bc[f] == FDTD_BC_NEIGHBOR) &&
        !(shell && h->cfg.bc[f] == FDTD_BC_PERIODIC && h->cfg.bc[f ^ 1] == FDTD_BC_PERIODIC)) return FDTD_F2_OFF_BOUNDARY;
  if ((h->g.pec_z0 != 0) != (h->cfg.bc[4] == FDTD_BC_PEC) || h->g.nx % 4 || h->g.nz < 2) return FDTD_F2_OFF_BOUNDARY;
  for (int a = 0; a < 3; ++a) if (h->mirror_wall[a] >= 0) return FDTD_F2_OFF_BOUNDARY;
  return 0;
}
bool fused2_eligible(const FdtdSolver* h) { return !any_pml(h) && fused2_why_not(h) == 0; }
// Can the pair (n, n + 1) be taken as far as the sources go?  0 = yes, else the reason.  The sweep applies the node table of ALL
// point-source lists or none: they must be all alive (then at most kMaxInj nodes — a dipole, a few; not a mode plane or a current
// sheet —, no H_y / H_z node left of a tile seam, no magnetic node together with absorber layers, and the table of all steps
// for magnetic nodes) or all spent (then nothing is injected and their number does not matter: a mode source or a TFSF box
// keeps single steps for the length of its pulse, the rest of the run goes out in pairs).  That is judged at step n; of step n + 1 one
// thing is asked as well: no list may end at n while another list's H side goes on (below).  `*alive`: the lists inject at step n.
int fused2_sources_why_not(const FdtdSolver* h, long long n, bool* alive = nullptr) {
  bool any_alive = false, any_spent = false;
  for (const PointSrc& s : h->psrc)
    if (s.has_nodes()) (s.alive(n) ? any_alive : any_spent) = true;
  if (alive) *alive = any_alive;
  for (const Tfsf& t : h->tfsf) if (n < t.n_steps) return FDTD_F2_OFF_TFSF;
  if (any_alive && any_spent) return FDTD_F2_OFF_SOURCES;
  if (!any_alive) return 0;
  // the pair (n, n + 1): the sweep takes the H-side terms of step n + 1 from the table row of ALL lists (InjP::val2) or from none.  A
  // list whose last step is n while an H side goes on at n + 1 would leave that H side without its term: single steps there
  bool ends = false, h_goes_on = false;
  for (const PointSrc& s : h->psrc)
    if (s.has_nodes()) { ends = ends || (s.alive(n) && !s.alive(n + 1)); h_goes_on = h_goes_on || (s.h.n > 0 && s.alive(n + 1)); }
  if (ends && h_goes_on) return FDTD_F2_OFF_SOURCES;
  if (h->src_nodes > kMaxInj) return FDTD_F2_OFF_SOURCES;
  if (h->src_h_nodes > 0 && !h->src_tab) return FDTD_F2_OFF_SOURCES;      // H-side nodes take their terms of step n+1 from the table only
  if (h->has_damp && h->src_h_nodes > 0) return FDTD_F2_OFF_H_SOURCE_ABSORBER;  // absorber layers are applied inside the sweep, H-side sources of step n in front of it
  if (h->src_h_on_seam) return FDTD_F2_OFF_SEAM_SOURCE;                    // the seam kernel rebuilds that value without the source term
  return 0;
}

// A time monitor whose record of a middle step the sweep can copy out on the way: every component of every cell of its box,
// a few hundred values at most (each costs every wave of its plane a scalar table entry).
bool fused2_capturable(const FdtdSolver* h, const Monitor& m) {
  if (m.kind != FDTD_MON_TIME || m.cells <= 0 || (long long)m.comps.size() * m.cells > kMaxCap) return false;
  const BoxP& b = m.box;
  return b.lo0 >= 0 && b.lo1 >= 0 && b.lo2 >= 0 && b.lo0 + b.nx <= h->g.nx && b.lo1 + b.ny <= h->g.ny && b.lo2 + b.nz <= h->g.nz;
}

// The monitors that record at step n or at step n + 1: the pair (n, n + 1) can go out as one sweep if they are all small
// time monitors (at most kPairMons).  The sweep copies their samples of the middle step (E^{n+1}, H^{n+1/2}) out; ONE launch
// behind it (pair_record_kernel) writes everything they record of the pair — E^n and H^{n-1/2} are still in the set the
// sweep read, H^{n+3/2} is in the set it wrote — so such a pair costs no record launch in front of the sweep.
// `box` (shell pairs): the bulk the sweep covers — a monitor that records at either step must lie inside it.
bool fused2_plan(const FdtdSolver* h, long long n, F2Plan* plan, const int* box_lo = nullptr, const int* box_hi = nullptr, bool dft_anywhere = false) {
  plan->mons.clear(); plan->dfts.clear(); plan->dft_when.clear();
  long long total = 0, dump = 0;
  for (size_t q = 0; q < h->mons.size(); ++q) {
    const Monitor& m = h->mons[q];
    bool at_n = false, at_m = false;
    for (size_t r = m.next; r < m.steps.size() && m.steps[r] <= n + 1; ++r) { at_n = at_n || m.steps[r] == n; at_m = at_m || m.steps[r] == n + 1; }
    if (!at_n && !at_m) continue;
    const BoxP& b = m.box;
    const bool inside = b.lo0 >= 0 && b.lo1 >= 0 && b.lo2 >= 0 && b.lo0 + b.nx <= h->g.nx && b.lo1 + b.ny <= h->g.ny && b.lo2 + b.nz <= h->g.nz;
    // (shell2 pairs: the shell's boxes copy the middle step out too — a DFT monitor may reach into the layers, as flux planes and mode
    //  monitors normally do; time monitors' samples come from the bulk sweep's node table only)
    if (box_lo && !(dft_anywhere && records_as_dft(m)) &&
        (b.lo0 < box_lo[0] || b.lo1 < box_lo[1] || b.lo2 < box_lo[2] || b.lo0 + b.nx > box_hi[0] ||
         b.lo1 + b.ny > box_hi[1] || b.lo2 + b.nz > box_hi[2])) return false;
    if (records_as_dft(m)) {
      // A DFT record at the FIRST step: E^n is taken in front of the sweep as always; its H terms need H^{n+1/2}.  A record at
      // the MIDDLE step: its E terms need E^{n+1}; its H terms, H^{n+3/2}, are in the write set afterwards.  The sweep copies
      // what is needed of the middle step out over the box (any size).
      if (!inside || m.cells <= 0) return false;
      for (int c : m.comps) if ((c >= 3 && at_n) || (c < 3 && at_m)) dump += m.cells;
      plan->dfts.push_back((int)q);
      plan->dft_when.push_back((at_n ? 1 : 0) | (at_m ? 2 : 0));
      continue;
    }
    if (!fused2_capturable(h, m) || m.comps.size() > 6) return false;
    total += (long long)m.comps.size() * m.cells;
    plan->mons.push_back((int)q);
  }
  return total <= kMaxCap && (int)plan->mons.size() <= kPairMons && (int)plan->dfts.size() <= kMaxDumps && dump <= (1LL << 26);
}

// the source terms of every step, formed once with the operations of point_source_kernel: [step][node], nodes in the order of
// the node tables (E nodes then H nodes of each list).  Rebuilt when lists were added.  0 = fine (src_tab may stay nullptr when
// the table would be too large: then the terms of step n are formed per pair and those of step n+1 go behind the launch)
int fused2_sources(FdtdSolver* h) {
  const GridP& g = h->g;
  if (h->inj_sources != h->psrc.size()) {
    h->f2_tables.clear();
    h->inj_sources = h->psrc.size();
    // the source terms of every step, formed once with the operations of point_source_kernel
    h->src_tab = nullptr;
    h->src_on_seam = false;
    h->src_h_on_seam = false;
    h->src_e_in_damp = false;
    long long nodes = 0, steps = 0;
    h->src_h_nodes = 0;
    for (const PointSrc& s : h->psrc) {
      nodes += s.e.n + s.h.n;
      h->src_h_nodes += s.h.n;
      if (s.has_nodes()) steps = std::max(steps, s.n_steps);
      for (long long t = 0; t < s.e.n; ++t) {
        const int i = (int)(s.e.host_cell[(size_t)t] % g.nx);
        h->src_on_seam = h->src_on_seam || (i % 256 == 255 && i + 1 < g.nx) || (i % 256 == 0 && i > 0);
        if (h->has_damp) {
          const long long cell = s.e.host_cell[(size_t)t];
          const int c3[3] = {i, (int)((cell % g.sxy) / g.nx), (int)(cell / g.sxy)};
          for (int a = 0; a < 3; ++a) h->src_e_in_damp = h->src_e_in_damp || c3[a] < h->damp_lo[a] || c3[a] >= h->damp_hi[a];
        }
      }
      for (long long t = 0; t < s.h.n; ++t) {
        const int i = (int)(s.h.host_cell[(size_t)t] % g.nx), c = s.h.host_comp[(size_t)t];
        h->src_h_on_seam = h->src_h_on_seam || (c != 3 && i % 256 == 255 && i + 1 < g.nx);
      }
    }
    h->src_nodes = nodes;
    if (nodes > 0 && nodes * steps <= (1LL << 24)) {
      if (dev_alloc(h, &h->src_tab, (size_t)(nodes * steps))) return -1;
      long long off = 0;
      for (const PointSrc& s : h->psrc)            // node order: E nodes then H nodes of each list (as the node table below)
        for (const PointSide* p : {&s.e, &s.h}) {
          if (p->n) launch_inject_table(h->stream, h->src_tab, nodes, off, p->wre, p->wim, p->wave, s.n_steps, (int)p->n);
          off += p->n;
        }
      h->src_tab_steps = steps; h->src_tab_nodes = nodes;
    }
  }
  return 0;
}

const F2Table* fused2_table(FdtdSolver* h, const F2Plan& plan, bool with_sources) {
  const GridP& g = h->g;
  if (fused2_sources(h)) return nullptr;
  for (const F2Table& t : h->f2_tables)
    if (t.with_sources == with_sources && t.mons == plan.mons && t.dfts == plan.dfts && t.dft_when == plan.dft_when) return &t;
  // the nodes of all E-side lists, sorted by plane; nodes of one plane keep their list order (a node two lists share
  // receives their terms in the order the source kernels would add them); the monitor samples of a plane follow them
  std::vector<std::array<int, 5>> ent;        // k, i, j, code, index
  int off = 0;
  for (const PointSrc& s : h->psrc) {
    if (!with_sources) break;          // (spent lists: nothing is injected, and a mode plane's 10^5 nodes would be walked per plane for nothing)
    for (const PointSide* p : {&s.e, &s.h})             // H-side nodes: codes 3 - 5, terms of step n+1 only (those of step n go out
      for (long long t = 0; t < p->n; ++t, ++off) {     // in front of the sweep, launch_sources)
        const long long cell = p->host_cell[(size_t)t];
        ent.push_back({(int)(cell / g.sxy), (int)(cell % g.nx), (int)((cell % g.sxy) / g.nx), (p == &s.h ? 3 : 0) + p->host_comp[(size_t)t] % 3, off});
      }
  }
  F2Table tb;
  tb.with_sources = with_sources;
  tb.mons = plan.mons;
  int coff = 0;
  for (size_t q = 0; q < plan.mons.size(); ++q) {
    Monitor& m = h->mons[(size_t)plan.mons[q]];
    tb.cap_off.push_back(coff);
    const BoxP& b = m.box;
    long long idx = 0;
    for (size_t ic = 0; ic < m.comps.size(); ++ic)
      for (long long t = 0; t < m.cells; ++t, ++idx) {
        const int lx = (int)(t % b.nx), ly = (int)((t / b.nx) % b.ny), lz = (int)(t / ((long long)b.nx * b.ny));
        ent.push_back({b.lo2 + lz, b.lo0 + lx, b.lo1 + ly, 8 + m.comps[ic], coff + (int)idx});
      }
    coff += (int)idx;
  }
  std::stable_sort(ent.begin(), ent.end(), [](const std::array<int, 5>& x, const std::array<int, 5>& y) {
    return x[0] != y[0] ? x[0] < y[0] : (x[3] >= 8) < (y[3] >= 8);
  });
  std::vector<int> start((size_t)g.nz + 2, 0);
  std::vector<int4> e4(std::max<size_t>(1, ent.size()));
  for (size_t q = 0; q < ent.size(); ++q) {
    start[(size_t)ent[q][0] + 1]++;
    e4[q].x = ent[q][1]; e4[q].y = ent[q][2]; e4[q].z = ent[q][3]; e4[q].w = ent[q][4];
  }
  for (int k = 0; k <= g.nz; ++k) start[(size_t)k + 1] += start[(size_t)k];
  if (dev_upload(h, &tb.start, (const int*)start.data(), start.size()) ||
      dev_upload(h, &tb.ent, (const int4*)e4.data(), e4.size())) return nullptr;
  // boxes of the DFT monitors that record at the first step, indexed by plane
  tb.dfts = plan.dfts; tb.dft_when = plan.dft_when;
  if (!plan.dfts.empty()) {
    std::vector<DumpBox> boxes;
    std::vector<std::vector<int>> per_plane((size_t)g.nz + 1);
    long long off = 0;
    for (size_t q = 0; q < plan.dfts.size(); ++q) {
      const Monitor& m = h->mons[(size_t)plan.dfts[q]];
      DumpBox bx{m.box.lo0, m.box.lo1, m.box.lo2, m.box.nx, m.box.ny, m.box.nz, {-1, -1, -1, -1, -1, -1}};
      const int when = plan.dft_when[q];
      for (int c : m.comps) if ((c >= 3 && (when & 1)) || (c < 3 && (when & 2))) { bx.off[c] = (int)off; off += m.cells; }
      tb.dft_off.push_back({bx.off[0], bx.off[1], bx.off[2], bx.off[3], bx.off[4], bx.off[5]});
      bool any = false;
      for (int c = 0; c < 6; ++c) any = any || bx.off[c] >= 0;
      if (!any) continue;                                                     // nothing of the middle step is needed
      for (int k = m.box.lo2; k < m.box.lo2 + m.box.nz; ++k) per_plane[(size_t)k].push_back((int)boxes.size());
      boxes.push_back(bx);
    }
    tb.dump_floats = off;
    if (!boxes.empty()) {
      std::vector<int> ds((size_t)g.nz + 2, 0), dl;
      for (int k = 0; k <= g.nz; ++k) { ds[(size_t)k] = (int)dl.size(); if (k < g.nz) for (int b : per_plane[(size_t)k]) dl.push_back(b); }
      ds[(size_t)g.nz + 1] = (int)dl.size();
      if (dl.empty()) dl.push_back(0);
      if (dev_upload(h, &tb.dstart, (const int*)ds.data(), ds.size()) || dev_upload(h, &tb.dlist, (const int*)dl.data(), dl.size()) ||
          dev_upload(h, &tb.dboxes, (const DumpBox*)boxes.data(), boxes.size())) return nullptr;
    }
  }
  h->f2_tables.push_back(tb);
  return &h->f2_tables.back();
}

// Tile classes of a launch shape of the two-step sweep (round 5): cls[tile] = 1 where any row segment the workgroup of that tile
// computes E for (its rows j0-2 .. j0+R, planes k0-1 .. k1) differs from the background word, 0 where the tile is background only —
// there the materials launch runs the plain sweep (fused2_step_kernel; the uniform coefficients ARE the table's entry 1: the same
// bits).
// `disp` (a launch that advances dispersive cells): class 2 where a row segment the workgroup visits holds one, 1 for other tiles with bodies.
// `src` (a launch that adds paged source terms): + 4 where a row segment the workgroup visits holds a source node — the other tiles run
// the instantiation without those lines (a launch over a uniform medium has this bit only).
const FdtdSolver::TileClasses* tile_classes(FdtdSolver* h, int W, int zc, const ClipP& box, int nbx, int nby, int nbz, bool disp = false, bool src = false) {
  const bool mats = h->mat4 && !h->roww_host.empty();
  if ((!mats && !src) || h->tile_split == 0) return nullptr;
  for (const auto& t : h->tile_cls)
    if (t.W == W && t.zc == zc && t.nbx == nbx && t.nby == nby && t.nbz == nbz && t.box.j0 == box.j0 && t.box.j1 == box.j1 &&
        t.box.k0 == box.k0 && t.box.k1 == box.k1 && t.disp == disp && t.src == src) return &t;
  const GridP& g = h->g;
  const int R = W - 3, nbx_all = (g.nx + 255) / 256;
  std::vector<unsigned char> cls((size_t)nbx * nby * nbz, 0);
  long long n_bg = 0;
  for (int tz = 0; tz < nbz; ++tz)
    for (int tx = 0; tx < nbx; ++tx)
      for (int ty = 0; ty < nby; ++ty) {
        const int k0 = box.k0 + tz * zc, k1 = std::min(k0 + zc, box.k1);
        const int j0 = box.j0 + ty * R;
        unsigned char c = 0;
        for (int k = std::max(k0 - 1, 0); mats && k <= std::min(k1, g.nz - 1) && !c; ++k)
          for (int j = std::max(j0 - 2, 0); j <= std::min(j0 + R, g.ny - 1); ++j)
            if (h->roww_host[((size_t)k * g.ny + j) * nbx_all + tx] != kBgWord) { c = 1; break; }
        if (disp && c && h->disp.seg.any(g, k0 - 1, k1, j0 - 2, j0 + R, tx, tx)) c = 2;
        n_bg += !c;
        if (src && h->spg.seg.any(g, k0 - 1, k1, j0 - 2, j0 + R, tx, tx)) c |= 4;
        cls[((size_t)tz * nbx + tx) * nby + ty] = c;
      }
  FdtdSolver::TileClasses e{W, zc, box, nbx, nby, nbz, nullptr, n_bg, (long long)cls.size(), disp, src};
  if (dev_upload(h, &e.dev, (const unsigned char*)cls.data(), cls.size())) return nullptr;
  h->tile_cls.push_back(e);
  return &h->tile_cls.back();
}

// steps n and n + 1 in one sweep: set a (E^n, H^{n-1/2}) -> set b (E^{n+2}, H^{n+3/2}).  The E-side sources of step n are
// applied inside the kernel; so are those of step n + 1 (*sources2_done) when their terms come from the table of all steps
// and no source node lies next to a seam — else the caller applies them afterwards.  The middle step is copied out for the
// monitors of `tb` (fused2_plan); pair_record (called by the caller behind the launch) writes their records.
// With `clip` the launch covers that box only (the bulk of a shell pair): nothing outside it is written, the E-side sources
// of step n + 1 are left to the caller, and the sets are NOT swapped (the shell launches beside it still name them).
// `use_disp`: the sweep subtracts the memory terms of the dispersive cells from E^{n+1} and leaves it for launch_ade2, which the
// caller issues behind the launch (and behind the sources / damping of step n + 1 it applies itself).  `e2_clip`: a clipped launch
// may apply the E-side sources of step n + 1 itself (the caller's ONE launch covers every source node).
// `sr`: paged source terms of this pair (the caller has filled them, spg_fill; the node table then lists no sources).
// `defer_ok` (plain_pair): the caller knows that nothing but the next plain pair will read the set this one writes — where the launch
// allows it too, seam_kernel leaves its values in the repair array (h->seam_pending) and the next launch's edge lanes take them there.
void flush_seams(FdtdSolver* h, hipStream_t st);
int launch_fused2(FdtdSolver* h, long long n, hipStream_t st, const F2Table* tb, bool* sources2_done, bool* damp2_done = nullptr,
                  const ClipP* clip = nullptr, bool use_disp = false, bool e2_clip = false, const SrcP& sr = SrcP{}, bool defer_ok = false) {
  const bool inject = tb->with_sources;      // (false: the lists are spent, or — shell pairs with z holes — their planes take single steps)
  const GridP& g = h->g;
  if (use_disp && !h->mat4) return fail(h, "launch_fused2: dispersive cells in a pair without the materials grid");
  if (ensure_second_set(h)) return -1;
  int W = 16, zc = 32;
  const ClipP box = clip ? *clip : ClipP{0, g.nx, 0, g.ny, 0, g.nz};
  fused2_shape(h, &W, &zc, (clip && h->comm) ? clip : nullptr);
  // (beside the shell launches of a shell pair shorter chunks do better — workgroups retire, and hand their CU to a shell
  //  workgroup, twice as often: 512^3 V2 inside one engine 16 x 16 1.206 / 1.219 ms per step, 16 x 24 1.225, 16 x 32 1.249 / 1.231,
  //  profiles/r4d)
  // (... up to 512^3; larger grids have tile rounds to spare and prefer the long chunks of the plain sweep: V2 at 768^3 117.6 /
  //  119.6 / 123.1 Gcells/s with 16 / 32 / 64 planes, at 1024^3 127.2 / 131.5 / 134.7, profiles/r4/r4u)
  if (clip && !h->comm && h->twostep_zc <= 0 && (long long)g.nx * g.ny * g.nz < (1LL << 28)) zc = std::min(zc, 16);
  zc = std::max(2, std::min(zc, box.k1 - box.k0));
  h->twostep_w_used = W; h->twostep_zc_used = zc;
  const int R = W - 3;
  const int nbx = (g.nx + 255) / 256, nby = (box.j1 - box.j0 + R - 1) / R;
  const int nbz = (box.k1 - box.k0 + zc - 1) / zc;
  const int n_seams = nbx - 1 + ((clip && h->cfg.bc[0] == FDTD_BC_PERIODIC) ? 1 : 0);        // (periodic x: the wrap is a seam too)
  if (!h->seam_buf && (nbx > 1 || h->cfg.bc[0] == FDTD_BC_PERIODIC) &&
      dev_alloc(h, &h->seam_buf, seam_scratch_floats(g, nbx) + seam_rep_floats(g, nbx))) return -1;
  if (!h->inj_val && dev_alloc(h, &h->inj_val, (size_t)kMaxInj)) return -1;
  if (!h->cap_val && dev_alloc(h, &h->cap_val, (size_t)kMaxCap)) return -1;
  InjP inj{};
  *sources2_done = false;
  {
    bool alive = false, alive2 = true;
    for (const PointSrc& s : h->psrc)
      if (inject && s.has_nodes()) { alive = alive || s.alive(n); alive2 = alive2 && s.alive(n + 1); }
    // (all lists alive or all spent: fused2_sources_uniform.  Spent lists add nothing — not + 0 — so their table is only
    //  walked when there are none or when they are alive: pairs with monitor samples AND spent sources are not taken, fdtd_run)
    if (alive && h->src_tab && n + 1 < h->src_tab_steps) {
      inj.val = h->src_tab + n * h->src_tab_nodes;
      if (alive2) {
        inj.val2 = h->src_tab + (n + 1) * h->src_tab_nodes;
        // (round 6: a node next to a seam no longer sends them behind the launch — seam_kernel adds the terms of the values it repairs)
        if (!clip || e2_clip) { inj.e2_in_sweep = 1; *sources2_done = true; }
      }
    } else if (alive) {
      int off = 0;
      for (const PointSrc& s : h->psrc) {
        if (s.e.n) launch_inject_values(st, h->inj_val + off, s.e.wre, s.e.wim, s.e.wave, n, (int)s.e.n);
        off += (int)(s.e.n + s.h.n);
      }
      inj.val = h->inj_val;
    }
    inj.n = (alive || !tb->mons.empty()) ? 1 : 0;
    inj.start = tb->start; inj.ent = tb->ent; inj.cap = h->cap_val;
    if (tb->dstart) {
      if (tb->dump_floats > h->dump_cap) {
        if (dev_alloc(h, &h->dump_buf, (size_t)tb->dump_floats, false)) return -1;
        h->dump_cap = tb->dump_floats;
      }
      inj.dstart = tb->dstart; inj.dlist = tb->dlist; inj.dboxes = tb->dboxes; inj.dump = h->dump_buf;
      inj.n = 1;
    }
  }
  // absorber layers: H^{n-1/2}, E^{n+1}, H^{n+1/2} are damped in registers; E^{n+2} too unless E-side sources of step n+1 still
  // have to be applied behind the launch (the damping follows the sources: then the caller damps, launch_damp)
  DampT dmp{};
  if (h->has_damp) {
    for (int a = 0; a < 3; ++a) { dmp.fb[a] = h->damp_fb[a]; dmp.fc[a] = h->damp_fc[a]; }
    const bool post_sources = e_sources_due(h, n + 1);
    // (... unless every E-side source node lies outside the layers: there the factor is exactly 1 — damp (E + s) == damp (E) + s bit
    //  for bit — and the sweep damps E^{n+2} itself.  The bench's dipole sits on the seam column 256 of a 512-cell row, which sent
    //  six damping launches over 40 % of the grid behind every pair: 20 % of the `va` step)
    dmp.e2 = (!post_sources || inj.e2_in_sweep || sr.sseg || !h->src_e_in_damp) ? 1 : 0;
    if (damp2_done) *damp2_done = dmp.e2 != 0;
  }
  const int total = nbx * nby * nbz;
  // tile order: runs of 32 tiles per XCD (the single sweep: 8) — inside engines at 512^3: runs of 8 0.7165, 16 0.7143, 32 0.7090,
  // 40 0.730, 64 0.726, plain order 0.7225 ms per step (profiles/r3zm)
  const int remap = h->xcd_remap < 0 ? 32 : h->xcd_remap;
  StepP sp = step_params(h);
  time_begin(h, 2, st);
  const MatP mp = mat_params(h);
  DispP dp{nullptr, nullptr, nullptr};
  if (use_disp) dp = DispP{h->disp.seg.dev, h->disp.cs, h->disp.e1};
  const bool damp = !clip && h->has_damp;
  SrcP sr_used = sr;
  if (h->whatif == 9 && !sr.sseg && !damp && (!use_disp || clip)) {
    // measuring aid (scripts/probe_bodies.py): the instantiation that adds paged source terms over a map WITHOUT any source segment —
    // every tile dispatches to the bodies the plain launch runs: what the larger kernel costs by itself (results unchanged)
    SrcPaged& S = h->spg;
    const size_t nseg = (size_t)g.nz * g.ny * ((g.nx + 255) / 256);
    if (!S.seg.dev && S.state != 1) {
      S.seg.host.assign(nseg, -1);
      SrcT tab{};
      if (dev_upload(h, &S.seg.dev, (const int*)S.seg.host.data(), nseg) || dev_upload(h, &S.tab, &tab, 1)) return -1;
    }
    if (S.seg.dev && S.state != 1) { sr_used.sseg = S.seg.dev; sr_used.t = S.tab; }
  }
  // the word of the launch (fdtd_fused2.hpp).  What-if variants: measuring aids, the vacuum sweep with part of its work skipped (19: the
  // sweep without its stores into the seam scratch, variant 9 of the kernel; option 9 itself is the map above)
  const int wv = h->whatif == 19 ? 9 : ((h->whatif >= 1 && h->whatif <= 15 && h->whatif != 9) ? h->whatif : 0);
  const auto word = [&](bool rep) {
    return fused2_opt(h->mem_hints != 0, h->mat4 != nullptr, !(tb->mons.empty() && (!tb->with_sources || h->src_h_nodes == 0) && !tb->dstart),
                      clip != nullptr, damp, use_disp, sr_used.sseg != nullptr, wv, rep, W);
  };
  // deferred seam repair: the sixteen-wave plain / materials / absorber sweep of the whole grid reads and leaves the compact array
  // (its sixteen-wave instantiation serves every workgroup size; by default only the launches that run it anyway defer)
  const bool rep_capable = n_seams > 0 && !clip && (W == 16 || h->seam_defer == 2) && fused2_rep_word(word(false));
  const int opt = word(rep_capable && (h->seam_pending || h->whatif == 17));
  const auto no_sweep = [&] { return fail(h, "launch_fused2: no instantiation of the sweep for opt 0x%x, %d waves", opt, W); };
  if (!fused2_instantiated(fused2_lb(W, opt), opt)) return no_sweep();       // (in front of everything that changes the handle's state)
  if (sr.sseg) { *sources2_done = true; h->spg.pairs++; }
  float* const rep_arr = h->seam_buf ? h->seam_buf + seam_scratch_floats(g, nbx) : nullptr;
  if (h->seam_pending && !rep_capable) flush_seams(h, st);      // (the set it flushes, h->f, is the one this launch reads)
  h->seam_pending = false;
  bool defer = defer_ok && rep_capable && h->seam_defer != 0 && h->whatif == 0;
  if (defer) {        // nothing may touch the set behind the seam kernel: E-side sources of step n + 1 and the damping of E^{n+2} are in the sweep, or absent
    if ((e_sources_due(h, n + 1) && !*sources2_done) || (h->has_damp && !dmp.e2)) defer = false;
  }
  const int blocks = remap ? ((total + 7) / 8) * 8 : total;
  // background-only tiles take the plain sweep inside the materials launch (fdtd_kernels2.hpp, tile classes)
  const FdtdSolver::TileClasses* tc = tile_classes(h, W, zc, box, nbx, nby, nbz, use_disp, sr_used.sseg != nullptr);
  const bool split = tc && (use_disp || sr_used.sseg || (tc->n_bg > 0 && (h->tile_split == 1 || 8 * tc->n_bg >= tc->n_all)));
  const bool launched = launch_fused2_step(Fused2Launch{st, W, opt, blocks, g, h->f, h->f2, sp, mp, zc, nbx, nby, nbz, remap, inj, h->seam_buf, dmp, box,
                                                        TileClassP{split ? tc->dev : nullptr}, dp, sr_used});
  time_end(h, st);
  if (!launched) return no_sweep();       // (a unit's case labels and fused2_instantiated expand the same lists)
  {
    const int64_t word = FDTD_SWEEP_WORD(fused2_lb(W, opt), opt, W);
    if (std::find(h->sweep_words.begin(), h->sweep_words.end(), word) == h->sweep_words.end()) h->sweep_words.push_back(word);
  }
  if (n_seams > 0 && !(rep_capable && (h->whatif == 16 || h->whatif == 17))) {
    time_begin(h, 4, st);
    launch_seams(st, g, h->f2, sp, mp, h->seam_buf, n_seams, dmp, box, inj, sr, (defer || (h->whatif == 18 && rep_capable)) ? rep_arr : nullptr);
    time_end(h, st);
  }
  if (use_disp) h->disp.pairs++;
  if (!clip) swap_sets(h);
  if (defer) { h->seam_pending = true; h->seam_deferred_pairs++; }
  return 0;
}
// the repair array into the seam columns of the current set, in front of whatever reads them there (kind 5 of the kernel timers)
void flush_seams(FdtdSolver* h, hipStream_t st) {
  if (!h->seam_pending) return;
  const int nbx = (h->g.nx + 255) / 256;
  time_begin(h, 5, st);
  launch_seam_flush(st, h->g, h->f, h->seam_buf + seam_scratch_floats(h->g, nbx), nbx - 1);
  time_end(h, st);
  h->seam_pending = false;
  h->seam_flushes++;
}

// ---- shell pairs: two steps per sweep on grids walled by CPML ------------------------------------------------------------
// An error made by ignoring a per-step feature travels one cell per half step, so after a step pair it is confined to the
// feature's cells plus a collar.  The CPML recursions live in slabs on the faces: the two-step sweep (plain formulas) advances
// the BULK  O = [lo + 2, hi0 - 1) per CPML axis (x rounded inwards to multiples of 4) — every intermediate value it forms for O
// lies in cells where the plain update is the exact one — and the SHELL (the rest: slabs + collar, 16 % of a 512^3 grid with 12
// layers) takes two single steps of the production kernels beside it, on the second stream:
//     step one   set A -> set T (third set)   over the shell grown by one cell into the bulk (what step two differentiates)
//                E-side sources of step n, H-side ones of step n + 1 on T
//     step two   set T -> set B               over the shell
// The shell is cut into z slabs (all rows: all-axes instantiation), y slabs between them (tile rows that meet a slab, the
// rows of the bulk excluded: x + y instantiation) and x strips between those (strip_step_kernel).  Bulk and shell read A and
// write disjoint cells of B: no order between them inside a pair.  psi is touched by the shell launches only (H-side
// ping-pong: parity p in step one, p ^ 1 in step two, back to p).  Same kernels / formulas as single steps: the same bits.
struct ShellGeom { int o0[3], o1[3]; };
bool shell_geometry(const FdtdSolver* h, ShellGeom* G) {
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  for (int a = 0; a < 3; ++a) {
    const PmlAxisDev& P = h->pml[a];
    const int lo = P.ns > 0 ? P.lo : 0, hi0 = P.ns > 0 ? P.hi0 : N[a];
    int o0 = lo > 0 ? lo + 2 : 0, o1 = hi0 < N[a] ? hi0 - 1 : N[a];
    // a periodic y / z axis: the bulk stays two cells clear of the wrap (what it reads then lies inside the grid; the shell's
    // single steps wrap as they always did); periodic x wraps inside the sweep
    if (a > 0 && h->cfg.bc[2 * a] == FDTD_BC_PERIODIC) { o0 = 2; o1 = N[a] - 2; }
    if (a == 0) { o0 = (o0 + 3) / 4 * 4; o1 = o1 / 4 * 4; }
    if (o1 - o0 < (a == 0 ? 16 : 8)) return false;        // (also: the rounded x ranges met, lo == hi0 == n)
    G->o0[a] = o0; G->o1[a] = o1;
  }
  return true;
}

void release_buf(FdtdSolver* h, void* p);
int ensure_third_set(FdtdSolver* h) {
  const GridP& g = h->g;
  if (h->f3.ex) return 0;
  const size_t fcount = (size_t)g.sxy * (g.nz + 2);
  if (!h->fbase3[0] && alloc_field_set(h, h->fbase3, fcount, 2)) {
    for (int c = 0; c < 6; ++c) { if (h->fbase3[c]) release_buf(h, h->fbase3[c]); h->fbase3[c] = nullptr; }
    return -1;
  }
  h->f3.ex = h->fbase3[0] + g.sxy; h->f3.ey = h->fbase3[1] + g.sxy; h->f3.ez = h->fbase3[2] + g.sxy;
  h->f3.hx = h->fbase3[3] + g.sxy; h->f3.hy = h->fbase3[4] + g.sxy; h->f3.hz = h->fbase3[5] + g.sxy;
  return 0;
}

// one x strip of a shell step: columns [ci0, ci1), rows [j0, j1), planes [k0, k1)
void launch_strip(FdtdSolver* h, const FieldP& src, const FieldP& dst, const PmlP* pm, int ci0, int ci1, int j0, int j1,
                  int k0, int k1, hipStream_t st) {
  if (ci1 <= ci0 || j1 <= j0 || k1 <= k0) return;
  StripP sp;
  sp.q = std::min(kStripMaxQ, (ci1 - ci0) / 4);             // lanes per row: the strip's width (16 columns: 4; 20: 5), 64 columns per x tile at most
  sp.xorg = ci0; sp.ci0 = ci0; sp.ci1 = ci1; sp.j0 = j0; sp.j1 = j1; sp.kbeg = k0; sp.kend = k1;
  sp.zchunk = h->strip_zc;
  const int slots = (64 / sp.q) * kStripWaves;
  sp.nbx = (ci1 - ci0 + 4 * sp.q - 1) / (4 * sp.q);
  sp.nby = (j1 - j0 + slots - 2) / (slots - 1);
  sp.nbz = (k1 - k0 + sp.zchunk - 1) / sp.zchunk;
  const int pmc = h->cfg.bc[4] == FDTD_BC_PMC;
  const dim3 grid((unsigned)(sp.nbx * sp.nby * sp.nbz)), block(64, kStripWaves);
  time_begin(h, 3, st);
  if (h->mat4 && h->strip_occ == 4) hipLaunchKernelGGL((strip_step_kernel<true, 4>), grid, block, 0, st, h->g, src, dst, step_params(h), mat_params(h), pm, sp, pmc);
  else if (h->mat4) hipLaunchKernelGGL((strip_step_kernel<true, 3>), grid, block, 0, st, h->g, src, dst, step_params(h), mat_params(h), pm, sp, pmc);
  else if (h->strip_occ == 4) hipLaunchKernelGGL((strip_step_kernel<false, 4>), grid, block, 0, st, h->g, src, dst, step_params(h), mat_params(h), pm, sp, pmc);
  else hipLaunchKernelGGL((strip_step_kernel<false, 3>), grid, block, 0, st, h->g, src, dst, step_params(h), mat_params(h), pm, sp, pmc);
  time_end(h, st);
}

// The bulk's planes: the box's z range minus the z HOLES — plane ranges that take single steps with the shell although they lie
// inside the box: the planes that hold dispersive cells (their ADE state advances every step), and, while the lists inject, the
// planes of sources the sweep cannot apply itself (a mode plane, a current sheet, the injection plane of a plane wave: more than
// kMaxInj nodes, or TFSF corrections) — each grown by two planes (the reach of what the sweep gets wrong by ignoring them).
struct ZPlan {
  int n = 0;                 // bulk intervals [a[i], b[i]), ascending
  int a[4] = {}, b[4] = {};
  bool ok = false;           // a plan exists and the cost model likes it
};
bool zplan_build(const FdtdSolver* h, const ShellGeom& G, bool source_holes, ZPlan* P) {
  std::vector<std::pair<int, int>> holes;
  for (const AdeGroup& a : h->ade) if (a.n > 0) holes.push_back({a.k0 - 2, a.k1 + 2});
  if (source_holes) for_each_source_side(h, [&](const auto& L, bool) { holes.push_back({L.k0 - 2, L.k1 + 2}); });
  std::sort(holes.begin(), holes.end());
  P->n = 0;
  int lo = G.o0[2];
  auto close = [&](int hi) {           // the bulk interval [lo, hi): kept when it is worth a launch
    if (hi - lo >= 8) {
      if (P->n == 4) return false;
      P->a[P->n] = lo; P->b[P->n] = hi; P->n++;
    }
    return true;
  };
  for (const auto& hz : holes) {
    if (hz.second <= lo) continue;
    if (hz.first >= G.o1[2]) break;
    if (hz.first > lo && !close(std::min(hz.first, G.o1[2]))) return false;
    lo = std::max(lo, hz.second);
  }
  if (lo < G.o1[2] && !close(G.o1[2])) return false;
  return P->n > 0;
}
// the part of the bulk interval i that belongs to someone else in a shell step that reaches `grow` planes into the bulk
inline void zplan_in(const ZPlan& P, int i, int grow, int nz, int* k0, int* k1) {
  *k0 = P.a[i] + (P.a[i] > 0 ? grow : 0);
  *k1 = P.b[i] - (P.b[i] < nz ? grow : 0);
}

// One step of the shell: set `src` -> set `dst`, H-side psi parity `parity`.  in[a] = [in0[a], in1[a]) (a = x, y): the part of
// axis a that belongs to someone else in this step (the bulk O in step two, O shrunk by one cell on its CPML sides in step one);
// along z the bulk's intervals of `P`, shrunk by `grow` planes each.
int launch_shell_step(FdtdSolver* h, const FieldP& src, const FieldP& dst, int parity, const int in0[3], const int in1[3],
                      int pml_in, hipStream_t st, const ZPlan& P, int grow) {
  const GridP& g = h->g;
  const int R = h->rows_f, nby_all = (g.ny + R - 1) / R;
  ShellSets sh{src, dst, parity, 0, 0};
  // z slabs and z holes: the planes outside the bulk's intervals, all rows (two plane ranges per launch)
  {
    int r0[6], r1[6], nr = 0, lo = 0;
    for (int i = 0; i < P.n; ++i) {
      int k0, k1;
      zplan_in(P, i, grow, g.nz, &k0, &k1);
      if (k0 > lo) { r0[nr] = lo; r1[nr] = k0; ++nr; }
      lo = k1;
    }
    if (lo < g.nz) { r0[nr] = lo; r1[nr] = g.nz; ++nr; }
    for (int q = 0; q < nr; q += 2)
      if (launch_fused_range(h, st, {.k0 = r0[q], .k1 = r1[q], .pml = pml_in, .k2_0 = q + 1 < nr ? r0[q + 1] : 0, .k2_1 = q + 1 < nr ? r1[q + 1] : 0, .edge = true, .sh = &sh})) return -1;
  }
  for (int i = 0; i < P.n; ++i) {
    int k0, k1;
    zplan_in(P, i, grow, g.nz, &k0, &k1);
    if (k1 <= k0) continue;
    // y slabs: the planes of the interval, the tile rows that hold a row outside in[1] (the rows inside it excluded)
    if (in0[1] > 0 || in1[1] < g.ny) {
      const int ty_a = in0[1] > 0 ? std::min(nby_all, (in0[1] + R - 1) / R) : 0;
      const int ty_c = in1[1] < g.ny ? std::max(ty_a, in1[1] / R) : nby_all;
      sh.ex_j0 = in0[1]; sh.ex_j1 = in1[1];
      if (launch_fused_range(h, st, {.k0 = k0, .k1 = k1, .pml = pml_in & 3, .ty_n = ty_a + (nby_all - ty_c), .ty_a = ty_a, .ty_gap = ty_c - ty_a, .edge = true, .sh = &sh})) return -1;
      sh.ex_j0 = sh.ex_j1 = 0;
    }
    // x strips: planes of the interval, rows of in[1], the columns outside in[0]
    if (in0[0] > 0 || in1[0] < g.nx) {
      const PmlP* pm = h->pml_blk[pml_in][parity][h->pml_e_parity];
      launch_strip(h, src, dst, pm, 0, in0[0], in0[1], in1[1], k0, k1, st);
      launch_strip(h, src, dst, pm, in1[0], g.nx, in0[1], in1[1], k0, k1, st);
    }
  }
  return 0;
}

bool any_periodic(const FdtdSolver* h) {
  for (int f = 0; f < 6; ++f) if (h->cfg.bc[f] == FDTD_BC_PERIODIC) return true;
  return false;
}
int shell_why_not(const FdtdSolver* h, ShellGeom* G, ZPlan* base, ZPlan* with_src) {
  const int why = fused2_why_not(h, false, true);
  if (why) return why;
  if (!any_pml(h) && !any_periodic(h) && h->ade.empty()) return FDTD_F2_OFF_PML;              // (nothing to do here: the plain pairs cover it)
  if (h->shell_on == 0) return FDTD_F2_OFF_PML;
  if (h->has_damp) return h->ade.empty() ? FDTD_F2_OFF_PML : FDTD_F2_OFF_ADE;   // absorber layers with CPML or dispersive media: single steps
  // the shell runs the CPML recursions inside its sweeps (all axes), as a one-GPU step does by default
  if (64 * (h->rows_f + 1) > 512 || (h->pml_fused >= 0 && (h->pml_fused & pml_in_sweep_mask(h)) != pml_in_sweep_mask(h))) return FDTD_F2_OFF_PML;
  if (!shell_geometry(h, G)) return FDTD_F2_OFF_PML;
  // Is it worth it?  A shell cell costs a single step's bytes and more (fields + psi, through the third set, in launches that
  // cannot fill the machine), twice per pair; a bulk cell costs half a single step's.  Measured on MI355X, 512^3 V2, each kernel
  // alone on the machine (profiles/r4/r4c_kernel_trace_shell_pair_one_stream.txt; scaled to a single step of 10.1 ps per cell):
  // the bulk's two steps 10.3 ps per cell (12 with materials), a slab cell 25 ps per step, a strip cell 42 ps per step (64-byte
  // pieces at a 2 KB stride), and the two streams overlap to about 0.9 of the sum.  V2 (shell: 16 % of the cells): predicted 0.89
  // of two single steps, measured 0.88-0.89 (r4n).  BASELINE config 3 laid out with x = 224 (strips: 13 % of the cells): predicted
  // 1.11, measured 1.14-1.16 — pairs LOSE there (r4o), as on the V2 problem at 320^3 (1.08).  shell_on = 1 forces pairs (tests).
  // Two plans: the bulk's planes with the z holes of the dispersive cells only (`base`), and with those of every source list
  // too (`with_src`: what a pair uses while lists inject that the sweep cannot apply itself).
  auto judge = [&](bool source_holes, ZPlan* P) {
    P->ok = false;
    if (!zplan_build(h, *G, source_holes, P)) return;
    if (h->shell_on != 1) {
      const double N[3] = {(double)h->g.nx, (double)h->g.ny, (double)h->g.nz};
      const double ox = G->o1[0] - G->o0[0], oy = G->o1[1] - G->o0[1];
      double oz = 0.0;
      for (int i = 0; i < P->n; ++i) oz += P->b[i] - P->a[i];
      const double all = N[0] * N[1] * N[2], bulk = ox * oy * oz;
      const double strips = (N[0] - ox) * oy * oz, slabs = all - bulk - strips;
      const double pair_ps = 0.9 * (bulk * (h->mat4 ? 12.0 : 10.3) + 2.0 * (slabs * 25.0 + strips * 42.0));
      const double single_ps = 2.0 * all * 10.1;
      if (pair_ps > 0.97 * single_ps) return;
    }
    P->ok = true;
  };
  judge(false, base);
  judge(true, with_src);
  if (!base->ok) return h->ade.empty() ? FDTD_F2_OFF_SHELL : FDTD_F2_OFF_ADE;
  return 0;
}

// ---- shell2 pairs (round 5): the shell advanced by shell2_step_kernel, two steps per sweep with psi carried --------------------
// The grid is cut into the bulk O (shell_geometry: clipped two-step sweep, plain formulas) and up to six boxes that
// shell2_step_kernel advances beside it — all of them read set A and the current psi sets and write disjoint cells of set B and of
// the other psi sets, so there is no order between any two launches of a pair, no third field set and no middle-step launches:
//   x strips   the columns outside O_x, ALL rows and planes (the corners with the y / z slabs included: all-axes recursions)
//   z slabs    the columns of O_x, all rows, the planes outside O_z
//   y slabs    the columns of O_x, the rows outside O_y, the planes of O_z
// Taken when CPML makes the shell (no absorber layers, no periodic z) and, while source lists inject, when every source node lies
// three or more cells inside O (the boxes apply no sources; the bulk sweep applies its own) — or on planes that become z holes.
// What the boxes cannot advance takes two single steps through set T beside them, psi routed through temporary sets
// (Run::shell2_pair): z holes (the planes of dispersive cells and of big source planes), the two rows on either side of a periodic
// y wrap.  A periodic x needs neither: the boxes' halo lanes hold the wrapped columns (fdtd_shell2.hpp) and there are no x strips.
struct Shell2Box { int i0, i1, j0, j1, k0, k1; bool strip; int axes; };
constexpr int kShell2MaxBoxes = 24;
// Every box is cut so that most of its cells meet the recursions of ONE axis (the middle of an x strip: x; a y slab: y; the
// middle rows of a z slab: z) — their instantiation carries 32 psi registers instead of 96 — and the edges and corners, where two
// or three slabs cross, go out as small boxes of the all-axes instantiation.
int shell2_boxes_by_axes(const FdtdSolver* h, const ShellGeom& G, Shell2Box out[kShell2MaxBoxes]);
// (z_lo, z_hi: the planes of the x strips and — where they reach beyond G's plane range — of the z slabs: the whole grid, or the
//  segment of one bulk interval when z holes cut the run of planes)
int shell2_boxes(const FdtdSolver* h, const ShellGeom& G, Shell2Box out[kShell2MaxBoxes], int z_lo = 0, int z_hi = -1) {
  if (z_hi < 0) z_hi = h->g.nz;
  if (h->shell2_on != 2 && h->shell2_on != 3) {      // the default: six boxes, all of the all-axes instantiation (one launch)
    const int nx = h->g.nx, ny = h->g.ny, nz = h->g.nz;
    int n = 0;
    (void)nz;
    // (a periodic y: the two rows next to the wrap on either side belong to nobody here — they take single steps beside the
    //  boxes, Run::shell2_pair — so the x strips and z slabs end there and there are no y slabs)
    const bool per_y = h->cfg.bc[2] == FDTD_BC_PERIODIC;
    const int r0 = per_y ? G.o0[1] : 0, r1 = per_y ? G.o1[1] : ny;
    if (G.o0[0] > 0) out[n++] = {0, G.o0[0], r0, r1, z_lo, z_hi, true, 7};
    if (G.o1[0] < nx) out[n++] = {G.o1[0], nx, r0, r1, z_lo, z_hi, true, 7};
    if (G.o0[2] > z_lo) out[n++] = {G.o0[0], G.o1[0], r0, r1, z_lo, G.o0[2], false, 7};
    if (G.o1[2] < z_hi) out[n++] = {G.o0[0], G.o1[0], r0, r1, G.o1[2], z_hi, false, 7};
    if (!per_y && G.o0[1] > 0) out[n++] = {G.o0[0], G.o1[0], 0, G.o0[1], G.o0[2], G.o1[2], false, 7};
    if (!per_y && G.o1[1] < ny) out[n++] = {G.o0[0], G.o1[0], G.o1[1], ny, G.o0[2], G.o1[2], false, 7};
    return n;
  }
  return shell2_boxes_by_axes(h, G, out);
}
int shell2_boxes_by_axes(const FdtdSolver* h, const ShellGeom& G, Shell2Box out[kShell2MaxBoxes]) {
  const int nx = h->g.nx, ny = h->g.ny, nz = h->g.nz;
  const int ox0 = G.o0[0], ox1 = G.o1[0], oy0 = G.o0[1], oy1 = G.o1[1], oz0 = G.o0[2], oz1 = G.o1[2];
  int n = 0;
  auto add = [&](int i0, int i1, int j0, int j1, int k0, int k1, bool strip, int axes) {
    if (i1 > i0 && j1 > j0 && k1 > k0) out[n++] = {i0, i1, j0, j1, k0, k1, strip, axes};
  };
  // x strips (all rows and planes): the z-slab planes and the y-slab rows of the planes between them as all-axes boxes, the rest x only
  for (int side = 0; side < 2; ++side) {
    const int i0 = side == 0 ? 0 : ox1, i1 = side == 0 ? ox0 : nx;
    if (i1 <= i0) continue;
    add(i0, i1, 0, ny, 0, oz0, true, 7);
    add(i0, i1, 0, ny, oz1, nz, true, 7);
    add(i0, i1, 0, oy0, oz0, oz1, true, 7);
    add(i0, i1, oy1, ny, oz0, oz1, true, 7);
    add(i0, i1, oy0, oy1, oz0, oz1, true, 1);
  }
  // z slabs (the bulk's columns, all rows): the y-slab rows as all-axes boxes, the rows between them z only
  for (int side = 0; side < 2; ++side) {
    const int k0 = side == 0 ? 0 : oz1, k1 = side == 0 ? oz0 : nz;
    if (k1 <= k0) continue;
    add(ox0, ox1, 0, oy0, k0, k1, false, 7);
    add(ox0, ox1, oy1, ny, k0, k1, false, 7);
    add(ox0, ox1, oy0, oy1, k0, k1, false, 4);
  }
  // y slabs (the bulk's columns and planes): y only
  add(ox0, ox1, 0, oy0, oz0, oz1, false, 2);
  add(ox0, ox1, oy1, ny, oz0, oz1, false, 2);
  return n;
}
// tile shape of one box: lanes per row q for `W` waves per workgroup — the shape that wastes the fewest lane-planes (row slots of
// the last tile row and the three halo slots, halo lanes and the last x tile's idle lanes, the two extra iterations per chunk)
void shell2_shape(const FdtdSolver* h, const Shell2Box& bx, int W, int zc_cap, Shell2P* out) {
  const GridP& g = h->g;
  const bool per_x = h->cfg.bc[0] == FDTD_BC_PERIODIC;          // (the row wraps: a halo lane on both sides, holding the wrapped columns)
  const int halo_l = (bx.i0 > 0 || per_x) ? 1 : 0, halo_r = (bx.i1 < g.nx || per_x) ? 1 : 0;
  const int lanes_w = (bx.i1 - bx.i0) / 4;
  const int L = lanes_w + halo_l + halo_r;                   // lanes a row needs: the written ones and a halo lane on every side that is no wall
  const int rows = bx.j1 - bx.j0, nzb = bx.k1 - bx.k0;
  Shell2P best{};
  double best_cost = 0.0;
  int forced_q = bx.strip ? 0 : h->shell2_qw;
  if (forced_q > 0 && (64 / std::max(3, std::min(forced_q, L))) * W < 4) forced_q = 0;      // (a shape without a row to write: by box)
  for (int q = 3; q <= kShell2MaxQ; ++q) {
    if (forced_q > 0 && q != std::max(3, std::min(forced_q, L))) continue;
    if (q > std::max(3, L)) break;
    const int S = (64 / q) * W;
    // (a box that starts on the y-min wall — a wall, not a periodic wrap — and fits one tile row without the two halo slots below: jlo = 0)
    const bool wall_lo = bx.j0 == 0 && h->cfg.bc[2] != FDTD_BC_PERIODIC && rows <= S - 1 && !h->no_jlo;
    const int jlo = wall_lo ? 0 : 2;
    const int R = S - 1 - jlo;
    if (R < 1) continue;
    // tiles overlap by two lanes: tile t holds lanes t (q - 2) ... t (q - 2) + q - 1 of the row; lv = the last lane that must come out right
    const int lv = halo_r ? L - 2 : L - 1, qv = halo_r ? q - 2 : q - 1;
    const int nbx = 1 + std::max(0, (lv - qv + q - 3) / (q - 2));
    const int nby = (rows + R - 1) / R;
    int zc = bx.strip ? h->shell2_zcs : h->shell2_zcw;
    if (zc <= 0) {
      // planes per workgroup: chunks of equal length, zc_cap planes at most (each chunk pays two extra iterations and a prologue:
      // 512^3 V2 inside one engine 8 planes 1.054, 16: 1.031 / 1.054, 32: 1.005 / 1.028, 64: 0.998 / 1.026 ms per step, profiles/r5);
      // the caller lowers the cap until the launch as a whole gives the machine two rounds of workgroups
      const int nch = std::max(1, (nzb + zc_cap - 1) / zc_cap);
      zc = (nzb + nch - 1) / nch;
    }
    zc = std::max(1, std::min(zc, nzb));
    const int nbz = (nzb + zc - 1) / zc;
    const double cost = (double)nbx * nby * nbz * (zc + 2.5) * W;          // wave-iterations of the launch
    if (best.q == 0 || cost < best_cost * 0.999) {
      best_cost = cost;
      best.q = q; best.xorg = bx.i0 - 4 * halo_l;
      best.ci0 = bx.i0; best.ci1 = bx.i1; best.j0 = bx.j0; best.j1 = bx.j1; best.k0 = bx.k0; best.k1 = bx.k1;
      best.jlo = jlo;
      best.zchunk = zc; best.nbx = nbx; best.nby = nby; best.nbz = nbz;
    }
  }
  *out = best;
}
// The boxes of the shell as ONE launch of the all-axes instantiation (the default): six launches one behind the other left the
// machine half empty between them (0.92 against 0.69 ms per 512^3 V2 pair alone on the machine, profiles/r5/r5e), and one launch
// per instantiation — x / y / z only at three waves per SIMD for 94 % of the cells, all axes for the edges and corners — lost
// more to the four half-empty launches than the third wave bought (0.84 ms, profiles/r5/r5f).  shell2_on = 2 / 3: one launch per
// instantiation / per box (measuring aids).
int shell2_box_paged(FdtdSolver* h, const Shell2Box& bx);
void launch_shell2_boxes(FdtdSolver* h, const Shell2Box* bx, int n, const PmlP* pm, hipStream_t st, const F2Table* tb, bool use_disp = false,
                         const SrcP& sr = SrcP{}) {
  const DispP dp = use_disp ? DispP{h->disp.seg.dev, h->disp.cs, h->disp.e1} : DispP{nullptr, nullptr, nullptr};
  // (the DFT monitors of the pair's plan that reach into the shell: the boxes copy the middle step out over them; the dump buffer was sized by launch_fused2)
  Shell2Dump dmp{};
  if (tb && tb->dstart && h->dump_buf) { dmp.dstart = tb->dstart; dmp.dlist = tb->dlist; dmp.dboxes = tb->dboxes; dmp.dump = h->dump_buf; }
  const bool by_axes = h->shell2_on == 2 || h->shell2_on == 3;
  for (int axes : {1, 4, 2, 7}) {
    if (!by_axes && axes != 7) continue;
    Shell2M mb{};
    const int W = std::max(1, std::min(8, (by_axes && axes != 7) ? h->shell2_ws : h->shell2_ww));
    auto flush = [&]() {
      if (mb.n == 0) return;
      time_begin(h, 3, st);
      launch_shell2_step(st, W, h->mat4 != nullptr, axes, h->g, h->f, h->f2, step_params(h), mat_params(h), pm, mb, dmp, dp, sr);
      time_end(h, st);
      mb = Shell2M{};
    };
    // planes per chunk: 32 at most, fewer while the boxes of this launch together make less than two rounds of workgroups
    int zc_cap = 32;
    for (; zc_cap > 8; zc_cap -= (zc_cap > 16 ? 8 : 4)) {
      long long wgs = 0;
      for (int q = 0; q < n; ++q) {
        if (by_axes && bx[q].axes != axes) continue;
        Shell2P sp{};
        shell2_shape(h, bx[q], W, zc_cap, &sp);
        wgs += (long long)sp.nbx * sp.nby * sp.nbz;
      }
      if (wgs >= 2 * 256 * (W <= 4 ? 2 : 1)) break;
    }
    for (int q = 0; q < n; ++q) {
      if (by_axes && bx[q].axes != axes) continue;
      shell2_shape(h, bx[q], W, zc_cap, &mb.box[mb.n]);
      mb.box[mb.n].paged = (sr.sseg || dp.dseg) ? shell2_box_paged(h, bx[q]) : 0;
      mb.first[mb.n + 1] = mb.first[mb.n] + mb.box[mb.n].nbx * mb.box[mb.n].nby * mb.box[mb.n].nbz;
      mb.n++;
      if (mb.n == kShell2Boxes || h->shell2_on == 3) flush();
    }
    flush();
  }
}
// every node of every point-source list three or more cells inside the bulk on the axes / sides that carry a shell
bool shell2_sources_deep(const FdtdSolver* h, const ShellGeom& G) {
  const GridP& g = h->g;
  const int N[3] = {g.nx, g.ny, g.nz};
  auto deep = [&](long long cell) {
    const int c[3] = {(int)(cell % g.nx), (int)((cell % g.sxy) / g.nx), (int)(cell / g.sxy)};
    for (int a = 0; a < 3; ++a) {
      if (G.o0[a] > 0 && c[a] < G.o0[a] + 3) return false;
      if (G.o1[a] < N[a] && c[a] >= G.o1[a] - 3) return false;
    }
    return true;
  };
  for (const PointSrc& s : h->psrc)
    for (const PointSide* p : {&s.e, &s.h})
      for (uint32_t cell : p->host_cell) if (!deep(cell)) return false;
  return true;
}
int shell2_why_not(const FdtdSolver* h, ShellGeom* G) {
  const int why = fused2_why_not(h, false, true);
  if (why) return why;
  if (!any_pml(h) || h->shell2_on == 0 || h->shell_on == 0) return FDTD_F2_OFF_PML;
  // periodic x (wraps through halo lanes) and y (its rows next to the wrap take single steps beside the boxes) — one launch only;
  // a periodic z would put holes on the grid's ends: the round-4 form
  if (h->cfg.bc[4] == FDTD_BC_PERIODIC) return FDTD_F2_OFF_BOUNDARY;
  if (any_periodic(h) && (h->shell2_on == 2 || h->shell2_on == 3)) return FDTD_F2_OFF_BOUNDARY;
  // (dispersive cells: their planes are z holes of the bulk, as in the round-4 form — Run::setup_pairs checks that they lie inside it)
  if (!h->ade.empty() && (h->shell2_on == 2 || h->shell2_on == 3)) return FDTD_F2_OFF_ADE;
  if (h->has_damp) return FDTD_F2_OFF_PML;
  if ((long long)h->g.sxy * 4 >= (1LL << 32)) return FDTD_F2_OFF_PML;           // (32-bit lane offsets inside a plane)
  if (!shell_geometry(h, G)) return FDTD_F2_OFF_PML;
  if (h->shell2_on < 1) {
    // Is it worth it?  (constants and their source: kShell2*Ps above)
    const double N[3] = {(double)h->g.nx, (double)h->g.ny, (double)h->g.nz};
    const double ox = G->o1[0] - G->o0[0], oy = G->o1[1] - G->o0[1], oz = G->o1[2] - G->o0[2];
    const double all = N[0] * N[1] * N[2], bulk = ox * oy * oz, strips = (N[0] - ox) * N[1] * N[2], wide = all - bulk - strips;
    const double pair_ps = kShell2Overlap * (bulk * (h->mat4 ? kShell2BulkMatPs : kShell2BulkPs) + wide * kShell2WidePs + strips * kShell2StripPs);
    if (pair_ps > 0.95 * 2.0 * all * 10.1) return FDTD_F2_OFF_SHELL;
  }
  return 0;
}

// Ring monitors: every complete record not consumed yet — records [reduced, next) of each ring — is turned into its part of the
// monitor's result and its slot is zeroed again (the H half-samples are accumulated into a record).  Issued on the stream the
// records were written on, behind them: no other edge.
// Flux-time monitors (fdtd_flux_time.hpp): one value of the series per record, all monitors in one launch (kFluxMaxJobs per launch).
// Sparse field-time monitors (fdtd_field_time.hpp): the values on the kept nodes, one launch per monitor.
// grid.x, grid.y of a launch over the kept nodes of the component slots `slot[0 .. n)` (for_each_kept_node), grid.z the caller's
dim3 tap_grid(const TapTables& T, const int* slot, int n, unsigned gz) {
  int nx = 1;
  long long rows = 1;
  for (int e = 0; e < n; ++e) {
    nx = std::max(nx, T.nt[slot[e]][0]);
    rows = std::max(rows, (long long)T.nt[slot[e]][1] * T.nt[slot[e]][2]);
  }
  return dim3((unsigned)((nx + 63) / 64), (unsigned)std::min<long long>((rows + kFieldTimeRows - 1) / kFieldTimeRows, kFieldTimeMaxRowBlocks), gz);
}
// launch K<S>, S = the handle's FDTD_OPT_AXIS_SHIFT, with the workgroup of for_each_kept_node
#define LAUNCH_TAP_KERNEL(K, h, grid, st, ...) \
  hipLaunchKernelGGL(((h)->axis_shift == 1 ? K<1> : (h)->axis_shift == 2 ? K<2> : K<0>), grid, dim3(64, kFieldTimeRows), 0, st, __VA_ARGS__)

void ring_drain(FdtdSolver* h, hipStream_t st) {
  size_t q = 0;
  while (q < h->mons.size()) {
    FluxLaunchP L{};
    int tiles = 0, cnt = 0;
    for (; q < h->mons.size() && L.n < kFluxMaxJobs; ++q) {
      Monitor& m = h->mons[q];
      if (m.form != MonForm::FluxRing || m.reduced >= m.next) continue;
      FluxMonP& p = L.m[L.n++];
      p = m.fp;
      p.r0 = (long long)m.reduced;
      p.cnt = (int)(m.next - m.reduced);
      tiles = std::max(tiles, p.tiles); cnt = std::max(cnt, p.cnt);
    }
    if (!L.n) break;
    dbg_sync(h);
    hipLaunchKernelGGL(flux_time_reduce_kernel, dim3(tiles, cnt, L.n), dim3(256), 0, st, L);
    hipLaunchKernelGGL(flux_time_final_kernel, dim3((cnt + 255) / 256, L.n), dim3(256), 0, st, L);
  }
  for (const Monitor& m : h->mons) {
    if (m.form != MonForm::SparseRing || m.reduced >= m.next) continue;
    dbg_sync(h);
    static const int all_slots[6] = {0, 1, 2, 3, 4, 5};
    const size_t per_launch = (size_t)65535 / m.comps.size();          // (grid z: record x component)
    for (size_t r = m.reduced; r < m.next; r += per_launch) {
      FieldTimeP p = m.gp;
      p.r0 = (long long)r;
      p.cnt = (int)std::min(per_launch, m.next - r);
      LAUNCH_TAP_KERNEL(field_time_gather_kernel, h, tap_grid(p.t, all_slots, p.n_comps, (unsigned)(p.cnt * p.n_comps)), st, p);
    }
  }
  for (Monitor& m : h->mons) {
    if (!has_ring(m) || m.reduced >= m.next) continue;
    const size_t rec_bytes = m.comps.size() * (size_t)m.cells * sizeof(float);
    const size_t s0 = m.reduced % m.ring, cnt = m.next - m.reduced, first = std::min(cnt, m.ring - s0);
    hipMemsetAsync(reinterpret_cast<char*>(m.data) + s0 * rec_bytes, 0, first * rec_bytes, st);
    if (cnt > first) hipMemsetAsync(m.data, 0, (cnt - first) * rec_bytes, st);
    m.reduced = m.next;
  }
}

// One record launch of a sparse DFT monitor (fdtd_field_dft.hpp): the entries of `r` — component slots and the boxes they are read
// from, the live fields or the sweep's dump — colocated onto the kept nodes and accumulated with the nf phases at `phase`.
// A lattice DFT monitor (fdtd_lattice_dft.hpp) likewise, the lanes along each component's lattice_lane_axis.
void launch_field_dft(FdtdSolver* h, const Monitor& m, const FieldDftSrc& r, const float2* phase, hipStream_t st) {
  if (m.form != MonForm::LatticeDft) {
    LAUNCH_TAP_KERNEL(field_dft_record_kernel, h, tap_grid(m.dp.t, r.slot, r.n, (unsigned)r.n), st, m.dp, r, phase);
    return;
  }
  const TapTables& T = m.dp.t;
  int nl = 1;
  long long rows = 1;
  for (int e = 0; e < r.n; ++e) {
    const int L = lattice_lane_axis(T, r.slot[e]);
    nl = std::max(nl, T.nt[r.slot[e]][L]);
    rows = std::max(rows, lattice_rows(T, r.slot[e], L));
  }
  const dim3 grid((unsigned)((nl + 63) / 64), (unsigned)std::min<long long>((rows + kFieldTimeRows - 1) / kFieldTimeRows, kFieldTimeMaxRowBlocks), (unsigned)r.n);
  LAUNCH_TAP_KERNEL(lattice_dft_record_kernel, h, grid, st, m.dp, r, phase);
}

// H-side source terms of step n act on H^{n-1/2} in place in FRONT of a pair's sweep: then the small time monitors of the pair take
// E^n and their first H half-sample in front of those (record_monitors at the top of the step) and pair_record adds the rest.
// Round 6: the H-side corrections of a TFSF box count too — since such boxes inject inside pairs (paged source terms) a probe on
// one of their H nodes recorded half the term of step n too much (1e-12 of the field on the pulse's rising edge: one random device
// case in 200, scripts/fuzz_round6.py seed 11 case 47).
bool h_terms_in_front(const FdtdSolver* h) {
  if (h->src_h_nodes > 0) return true;
  for (const Tfsf& t : h->tfsf) if (t.h.n) return true;
  return false;
}
// behind the sweep of the pair (n, n + 1) (the sets are swapped: h->f2 = what it read, h->f = what it wrote): everything the
// monitors of `tb` record of steps n and n + 1, in one launch
void pair_record(FdtdSolver* h, const F2Table* tb, long long n, hipStream_t st) {
  dbg_sync(h);
  // DFT monitors: a record at step n took E^n in front of the sweep — its H terms from the sweep's copy of H^{n+1/2}; a record at
  // step n+1 takes its E terms from the copy of E^{n+1} here and its H terms (H^{n+3/2}) from the write set, record_monitors
  for (size_t q = 0; q < tb->dfts.size(); ++q) {
    Monitor& m = h->mons[(size_t)tb->dfts[q]];
    for (int pass = 0; pass < 2; ++pass) {
      if (m.next >= m.steps.size() || m.steps[m.next] != n + pass) continue;
      const float2* phase = (const float2*)((pass == 0 ? m.phase_h : m.phase_e) + (long long)m.next * m.nf);
      if (m.form == MonForm::SparseDft || m.form == MonForm::LatticeDft) {      // the dump holds the whole box of each component, contiguous
        FieldDftSrc s{};
        s.sy = m.box.nx; s.sz = (long long)m.box.nx * m.box.ny;
        for (size_t ic = 0; ic < m.comps.size(); ++ic)
          if ((m.comps[ic] >= 3) == (pass == 0)) { s.slot[s.n] = (int)ic; s.f[s.n] = h->dump_buf + tb->dft_off[q][(size_t)m.comps[ic]]; s.n++; }
        if (s.n > 0) launch_field_dft(h, m, s, phase, st);
      } else {
        DftDumpP r{};
        for (size_t ic = 0; ic < m.comps.size(); ++ic)
          if ((m.comps[ic] >= 3) == (pass == 0)) { r.slot[r.n] = (int)ic; r.off[r.n] = tb->dft_off[q][(size_t)m.comps[ic]]; r.n++; }
        if (r.n > 0)
          launch_dft_record_dump(st, r, h->dump_buf, reinterpret_cast<float2*>(m.data), m.cells, (long long)m.comps.size() * m.cells, phase, m.nf);
      }
      if (pass == 0) m.next++;
    }
  }
  if (tb->mons.empty()) return;
  PairRecP r{};
  r.pre_done = h_terms_in_front(h);            // (then fdtd_run has not skipped them at the top of the step)
  long long max_cells = 0;
  for (size_t q = 0; q < tb->mons.size(); ++q) {      // rings: room for the (at most two) records of this pair
    const Monitor& m = h->mons[(size_t)tb->mons[q]];
    if (!has_ring(m)) continue;
    size_t last = m.next;
    if (last < m.steps.size() && m.steps[last] == n) ++last;
    if (last < m.steps.size() && m.steps[last] == n + 1) ++last;
    if (last > m.next && last - 1 - m.reduced >= m.ring) { ring_drain(h, st); break; }
  }
  for (size_t q = 0; q < tb->mons.size(); ++q) {
    Monitor& m = h->mons[(size_t)tb->mons[q]];
    const long long rs = (long long)m.comps.size() * m.cells;
    r.box[q] = m.box;
    r.nc[q] = (int)m.comps.size();
    for (size_t ic = 0; ic < m.comps.size(); ++ic) r.comp[q][ic] = m.comps[ic];
    r.cap_off[q] = tb->cap_off[q];
    if (m.next < m.steps.size() && m.steps[m.next] == n) { r.out_n[q] = reinterpret_cast<float*>(m.data) + m.slot(m.next) * rs; m.next++; }
    if (m.next < m.steps.size() && m.steps[m.next] == n + 1) { r.out_m[q] = reinterpret_cast<float*>(m.data) + m.slot(m.next) * rs; m.next++; }
    max_cells = std::max(max_cells, m.cells);
  }
  r.n_mon = (int)tb->mons.size();
  launch_pair_record(st, r, max_cells, h->g, h->f2, h->f, h->cap_val);
}

// Placement of the field arrays.  Where the twelve arrays land in device memory moves the sweep by up to 15 % (DESIGN.md
// section 7; 1.08 ... 1.24 ms per 512^3 step over the 40 engines of profiles/r03d-r03t) and nothing in HIP steers it — but
// it can be sampled: before its first large run an engine allocates up to `placement_tries` further sets of the
// twelve arrays, times two PAIRS of plain sweeps (a -> b, b -> a: what a run does) on a copy of the live fields in each, and
// keeps the fastest set, copying the fields over.  Costs ten-odd sweeps and, for their duration, twice the field memory
// (skipped when that is not free).  For fused runs of at least 2^24 cells (2^22 per rank on z-slabs).  Measured (profiles/
// r03u_probe_placement_probe.jsonl, 10 engines, 3 candidates each): the set kept is 0.8 ... 8.1 % faster than the first
// allocations (mean 4 %), and the first allocations never won.
// What a run does: PAIRS of sweeps, set a -> b then b -> a.  The two directions read and write different arrays and differ
// in speed with the placement (one-directional timing said 1.094 ms per sweep where the run then took 1.146 ms per step,
// profiles/r3j), so both are timed: one warm-up pair, two timed pairs.  Advances the fields of the set it runs on.
float time_sweep_pairs(FdtdSolver* h, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  // a run the two-step sweep covers is timed on THAT kernel (its access pattern — 16 rows per workgroup, 32-plane chunks — is
  // not the single sweep's): launches without sources or monitor samples, set a -> b -> a as in the run
  const F2Table* tb = nullptr;
  if (fused2_eligible(h)) { F2Plan none; tb = fused2_table(h, none, false); }
  for (int k = 0; k < 6; ++k) {
    if (k == 2) hipEventRecord(e0, st);
    if (tb) {
      bool unused = false;
      if (launch_fused2(h, (1LL << 60), st, tb, &unused)) return -1.f;        // (a step no source list reaches: nothing is added)
    } else {
      if (launch_fused_range(h, st, {.k0 = 0, .k1 = h->g.nz})) return -1.f;
      swap_sets(h);
    }
  }
  hipEventRecord(e1, st);
  if (hipEventSynchronize(e1) != hipSuccess) return -1.f;
  float ms = 0.f;
  hipEventElapsedTime(&ms, e0, e1);
  return ms;
}
void set_field_views(FdtdSolver* h) {
  const long long o = h->g.sxy;
  h->f.ex = h->fbase[0] + o; h->f.ey = h->fbase[1] + o; h->f.ez = h->fbase[2] + o;
  h->f.hx = h->fbase[3] + o; h->f.hy = h->fbase[4] + o; h->f.hz = h->fbase[5] + o;
  h->f2.ex = h->fbase2[0] + o; h->f2.ey = h->fbase2[1] + o; h->f2.ez = h->fbase2[2] + o;
  h->f2.hx = h->fbase2[3] + o; h->f2.hy = h->fbase2[4] + o; h->f2.hz = h->fbase2[5] + o;
}
void release_buf(FdtdSolver* h, void* p) {
  for (size_t i = 0; i < h->bufs.size(); ++i)
    if (h->bufs[i].p == p) {
      hipFree(p);
      h->stats.device_bytes -= (int64_t)h->bufs[i].bytes;
      h->bufs.erase(h->bufs.begin() + (long)i);
      return;
    }
}
int probe_placement(FdtdSolver* h, hipStream_t st) {
  h->placement_done = true;
#ifdef FDTD_PLACEMENT_PROBE
  return 0;                                      // (measurement build: the arrays may live in one pooled allocation)
#else
  if (ensure_second_set(h)) return -1;
  const size_t fcount = (size_t)h->g.sxy * (h->g.nz + 2);
  const size_t need = 12 * fcount * sizeof(float);
  const int flags = h->cfg.flags;
  h->cfg.flags &= ~FDTD_FLAG_TIME_KERNELS;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {      // no timing, no probe: keep what we have
    if (e0) hipEventDestroy(e0);
    (void)hipGetLastError();
    h->cfg.flags = flags;
    return 0;
  }
  // Every set is timed on the SAME data — a copy of the live fields — in the mode a run uses (time_sweep_pairs); the
  // live set is timed in place, once, and restored from the first candidate's copy.
  float best = -1.f;
  float* cur[12];                                 // the set that holds the fields: at most this one and one candidate exist
  for (int c = 0; c < 6; ++c) { cur[c] = h->fbase[c]; cur[6 + c] = h->fbase2[c]; }
  auto copy6 = [&](float* const* dst, float* const* src) -> int {
    for (int c = 0; c < 6; ++c)
      if (hipMemcpyAsync(dst[c], src[c], fcount * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(h, "probe_placement: copy failed");
    return 0;
  };
  int rc = 0;
  // (round 6: candidates that lose are HELD until the probe ends — freed at once, their blocks came straight back as the next
  //  candidate and the probe timed the same placement again; up to 8 tries)
  std::vector<float*> held;
  for (int t = 0; t < h->placement_tries && t < 8 && !rc; ++t) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + need / 4) break;
    float* cand[12] = {};
    bool ok = true;
    for (int c = 0; c < 12 && ok; ++c) ok = dev_alloc(h, &cand[c], fcount) == 0;
    if (!ok) {                                    // out of memory after all: give back what was taken
      for (float* q : cand) if (q) release_buf(h, q);
      (void)hipGetLastError();
      h->err.clear();
      break;
    }
    auto drop_cand = [&]() { for (int c = 0; c < 12; ++c) held.push_back(cand[c]); };
    // dev_alloc zero-fills on the NULL stream, which this engine's non-blocking stream does not wait for: without this the
    // memset of a candidate could land AFTER the copy below and the "restored" fields came back partly zero (caught by
    // tests/test_gpu_production_path.py on the first visit with this probe, profiles/r3l)
    if (hipDeviceSynchronize() != hipSuccess) { drop_cand(); rc = fail(h, "probe_placement: %s", hipGetErrorString(hipGetLastError())); break; }
    rc = copy6(cand, cur);                        // the live fields (E, H of the current set), ghost planes included
    if (!rc && best < 0.f) {                      // the incumbent, in place; its fields come back from the copy
      best = time_sweep_pairs(h, st, e0, e1);
      h->placement_ms[0] = best;
      if (best < 0.f) rc = -1;
      if (!rc) rc = copy6(cur, cand);
    }
    if (rc) { drop_cand(); break; }
    for (int c = 0; c < 6; ++c) { h->fbase[c] = cand[c]; h->fbase2[c] = cand[6 + c]; }
    set_field_views(h);
    const float ms = time_sweep_pairs(h, st, e0, e1);
    for (int c = 0; c < 6; ++c) { h->fbase[c] = cur[c]; h->fbase2[c] = cur[6 + c]; }
    set_field_views(h);
    h->placement_ms[t + 1] = ms;
    h->placement_tried = t + 1;
    if (ms < 0.f) { drop_cand(); rc = -1; break; }
    // The candidate wins only by a clear margin.  Measured on 8 engines of one process (profiles/r3k): moves for a 0.6 ... 1.8 %
    // advantage in the probe ended 0.6 ... 2 % SLOWER in the run that followed, moves for 3.4 % and 5.8 % ended 2.6 % and
    // 4.5 % faster (first allocations 1.113 / 1.145 ms per step -> 1.084 / 1.093): the probe is there to escape a bad
    // placement, not to polish a good one.
    if (ms < 0.98f * best) {
      rc = copy6(cand, cur);
      if (!rc) rc = copy6(cand + 6, cur + 6);
      if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(h, "probe_placement: %s", hipGetErrorString(hipGetLastError()));
      if (rc) { drop_cand(); break; }
      for (int c = 0; c < 12; ++c) { held.push_back(cur[c]); cur[c] = cand[c]; }
      best = ms;
      h->placement_kept = t + 1;
    } else {
      if (hipStreamSynchronize(st) != hipSuccess) rc = fail(h, "probe_placement: %s", hipGetErrorString(hipGetLastError()));
      drop_cand();
    }
  }
  for (int c = 0; c < 6; ++c) { h->fbase[c] = cur[c]; h->fbase2[c] = cur[6 + c]; }
  set_field_views(h);
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(h, "probe_placement: %s", hipGetErrorString(hipGetLastError()));
  for (float* q : held) release_buf(h, q);
  if (getenv("FDTD_PLACEMENT_LOG")) {
    fprintf(stderr, "[placement] kept %d of 1 + %d:", h->placement_kept, h->placement_tried);
    for (int t = 0; t <= h->placement_tried; ++t) fprintf(stderr, " %.3f", h->placement_ms[t]);
    fprintf(stderr, " ms\n");
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  h->cfg.flags = flags;
  return rc;
#endif
}

// Tile-shape autotuning of the fused sweep.  Which (rows, z-chunk) shape is fastest depends on how
// the tile count quantises onto 256 CUs x 3 workgroups and on the slab height (profiles/
// r01g_probe_geometry.jsonl: 107 .. 111 Gcells/s across shapes at 512^3; a 64-plane slab prefers
// taller chunks).  The sweep reads set A and writes set B only, so timing it has no side effect
// and — the arithmetic being independent of the launch geometry — no effect on the results.
int autotune_fused(FdtdSolver* h, hipStream_t st) {
  h->tuned = true;
  const int nz = h->g.nz;
  if (ensure_second_set(h)) return -1;
  const int flags = h->cfg.flags;
  h->cfg.flags &= ~FDTD_FLAG_TIME_KERNELS;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const int rows_c[2] = {3, 2};
  const int zc_c[4] = {16, 24, 32, 8};
  int best_r = h->rows_f, best_z = h->zchunk_f;
  float best = 1e30f;
  for (int r : rows_c)
    for (int z : zc_c) {
      if (z > nz && z != 16) continue;
      h->rows_f = r; h->zchunk_f = z;
      if (launch_fused_range(h, st, {.k0 = 0, .k1 = nz})) return -1;             // warm-up (instruction cache, TLB)
      hipEventRecord(e0, st);
      for (int k = 0; k < 2; ++k) if (launch_fused_range(h, st, {.k0 = 0, .k1 = nz})) return -1;
      hipEventRecord(e1, st);
      if (hipEventSynchronize(e1) != hipSuccess) break;
      float ms = 0.f;
      hipEventElapsedTime(&ms, e0, e1);
      if (ms < best) { best = ms; best_r = r; best_z = z; }
    }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  h->rows_f = best_r; h->zchunk_f = best_z;
  h->cfg.flags = flags;
  return 0;
}

// two spins of 200 us, one on each stream: 1 = they ran side by side, 0 = one after the other (one hardware queue), -1 = error
int streams_run_side_by_side(FdtdSolver* h, hipStream_t a, hipStream_t b) {
#if defined(__HIPCC__)
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device) != hipSuccess || khz <= 0) khz = 100000;
  const long long ticks = (long long)khz / 5;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) return -1;
  int res = -1;
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, 0LL);
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, 0LL);
  if (hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess) {
    hipEventRecord(e0, a);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    hipEventRecord(e1, a);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    hipEventRecord(e2, b);
    if (hipEventSynchronize(e1) == hipSuccess && hipEventSynchronize(e2) == hipSuccess) {
      float t1 = 0.f, t2 = 0.f;
      hipEventElapsedTime(&t1, e0, e1);
      hipEventElapsedTime(&t2, e0, e2);
      res = std::max(t1, t2) < 0.32f ? 1 : 0;
    }
  }
  hipEventDestroy(e0); hipEventDestroy(e1); hipEventDestroy(e2);
  return res;
#else
  (void)h; (void)a; (void)b;
  return 1;
#endif
}
// the third stream of CPML slab-rank pairs (the shell's boxes beside the bulk and the cut planes' hole): one that shares a hardware queue
// with neither of the engine's two streams — fresh streams are tried, the rejected ones held meanwhile (the runtime hands a new stream the
// least-loaded queue); none found: box_stream stays null and the boxes keep their place in front of the bulk.  Called between runs' launches
// only at the first such pair (it synchronises the two streams).
int make_box_stream(FdtdSolver* h) {
  h->box_stream_tried = true;
  std::vector<hipStream_t> rejected;
  hipStream_t found = nullptr;
  for (int attempt = 0; attempt < 6 && !found; ++attempt) {
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
    const int a = streams_run_side_by_side(h, s, h->stream), b = a == 1 ? streams_run_side_by_side(h, s, h->comm_stream) : 0;
    if (a == 1 && b == 1) found = s; else rejected.push_back(s);
    if (a < 0 || b < 0) break;
  }
  for (hipStream_t r : rejected) hipStreamDestroy(r);
  (void)hipGetLastError();
  h->box_stream = found;
  h->box_stream_attempts = (int)rejected.size() + (found ? 1 : 0);
  if (found) {
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_box, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_box_in, hipEventDisableTiming));
  }
  return 0;
}
// Do the engine's two streams really run concurrently?  The HIP runtime multiplexes a process's streams onto
// $GPU_MAX_HW_QUEUES hardware queues (default 4); two streams that land on ONE queue execute their launches one after
// the other.  For this engine that is a silent 3x cliff: the boundary chunks and the interior sweep of a z-slab step
// (0.83 instead of 0.28 ms, profiles/r04u), the edge and interior launches of a CPML step.  So it is MEASURED, once,
// before the first run that uses both streams: a 200 us spin kernel on each; if the pair takes two spins instead of one,
// a fresh second stream is tried (the runtime gives a new stream the least-loaded queue of its priority class), a few
// times over; if none overlaps, the engine uses ONE stream for both roles and says so in FdtdStats.stream_overlap.
int probe_stream_overlap(FdtdSolver* h) {
  if (h->stream_overlap != 0) return 0;
#if defined(__HIPCC__)
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device) != hipSuccess || khz <= 0) khz = 100000;
  const long long ticks = (long long)khz / 5;                 // 200 us of the constant-rate clock
  hipEvent_t e0, e1, e2;
  HIPCHK(h, hipEventCreate(&e0));
  HIPCHK(h, hipEventCreate(&e1));
  HIPCHK(h, hipEventCreate(&e2));
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
  std::vector<hipStream_t> rejected;
  int rc = 0;
  bool ok = false;
  for (int attempt = 0; attempt < 6 && !rc; ++attempt) {
    hipStream_t a = h->stream, b = h->comm_stream;
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, 0LL);       // (code object resident, queues awake)
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, 0LL);
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) { rc = fail(h, "probe_stream_overlap: %s", hipGetErrorString(hipGetLastError())); break; }
    hipEventRecord(e0, a);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    hipEventRecord(e1, a);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    hipEventRecord(e2, b);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventSynchronize(e2) != hipSuccess) { rc = fail(h, "probe_stream_overlap: %s", hipGetErrorString(hipGetLastError())); break; }
    float t1 = 0.f, t2 = 0.f;
    hipEventElapsedTime(&t1, e0, e1);
    hipEventElapsedTime(&t2, e0, e2);
    if (std::max(t1, t2) < 0.32f) { ok = true; break; }      // one spin (0.2 ms) + launch latencies; two spins would be >= 0.4
    // serialised: another second stream
    hipStream_t fresh = nullptr;
    if (hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, attempt % 2 ? least : greatest) != hipSuccess) break;
    rejected.push_back(h->comm_stream);
    h->comm_stream = fresh;
    h->stream_retries++;
  }
  for (hipStream_t r : rejected) hipStreamDestroy(r);
  hipEventDestroy(e0); hipEventDestroy(e1); hipEventDestroy(e2);
  if (rc) return rc;
  if (ok) { h->stream_overlap = 1; return 0; }
  // fallback: one stream carries both roles (correct — every cross-stream edge becomes stream order — just not overlapped)
  hipStreamDestroy(h->comm_stream);
  h->comm_stream = h->stream;
  h->streams_shared = true;
  h->stream_overlap = -1;
  std::fprintf(stderr, "libfdtd_hip: the engine's two HIP streams do not run concurrently (shared hardware queue; "
                       "GPU_MAX_HW_QUEUES too low for this process?) - using one stream\n");
  return 0;
#else
  return 0;        // (the emulator runs every launch to completion: nothing to measure)
#endif
}

// periodic z, fused sweep: the prologue recomputes H^{n+1/2}[-1] from ghost copies of E (all three
// components) and H_x, H_y of plane nz-1; the top plane needs E_x, E_y of plane 0
// PMC on plus faces: refresh the mirror images beyond the walls (start of a step: E^n, H^{n-1/2} are complete)
// (k0, k1): the planes of this call — x / y walls are refreshed plane by plane; a z wall (the last rank's: images in its last two
//  planes, of the two below them) with the call that holds all four of its planes (fdtd_run checks that one does)
void fill_mirror(FdtdSolver* h, hipStream_t st, int k0 = 0, int k1 = -1) {
  dbg_sync(h);
  const GridP& g = h->g;
  if (k1 < 0) k1 = g.nz;
  if (k1 <= k0) return;
  for (int a = 0; a < 3; ++a) {
    const int N = h->mirror_wall[a];
    if (N < 0) continue;
    if (a == 2 && !(k0 <= N - 2 && N + 2 <= k1 && k0 >= 0 && k1 <= g.nz)) continue;
    const long long lines = (a == 0) ? (long long)g.ny * (k1 - k0) : (a == 1 ? (long long)g.nx * (k1 - k0) : g.sxy);
    hipLaunchKernelGGL(mirror_fill_kernel, dim3(nblk(lines)), dim3(256), 0, st, g, h->f, a, N, k0, k1 - k0);
  }
}

// one xy-plane device to device: a copy (the runtime's blit), or a kernel node while a graph is being captured
void copy_plane(FdtdSolver* h, float* dst, const float* src, hipStream_t st) {
  const long long pc = (long long)h->cfg.nx * h->cfg.ny;
  if (h->step_dev_mode) hipLaunchKernelGGL(copy_kernel, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, st, dst, src, pc);
  else hipMemcpyAsync(dst, src, pc * 4, hipMemcpyDeviceToDevice, st);
}
void fill_ghost_fused(FdtdSolver* h, hipStream_t st, const FieldP* fs = nullptr) {
  dbg_sync(h);
  if (h->cfg.bc[4] != FDTD_BC_PERIODIC) return;
  const FieldP F = fs ? *fs : h->f;
  const long long pc = plane_cells(h);
  const long long top = (long long)(h->g.nz - 1) * pc;
  float* lo[5] = {F.ex, F.ey, F.ez, F.hx, F.hy};
  for (float* p : lo) copy_plane(h, p - pc, p + top, st);
  copy_plane(h, F.ex + (long long)h->g.nz * pc, F.ex, st);
  copy_plane(h, F.ey + (long long)h->g.nz * pc, F.ey, st);
}

// slabs of one axis: E-side ranges [0,n_lo) and [N-n_hi+1,N); H-side [0,n_lo) and [N-n_hi,N)
// Axis order: H side x, y, z; E side y, z, x — so that a sweep that folds only the y and z
// recursions into the fused kernel (x stays a slab kernel before / after it) sums in the same order.
void launch_pml(FdtdSolver* h, bool e_side, int kbeg, int kend, hipStream_t st, int axes = 7) {
  dbg_sync(h);
  const GridP& g = h->g;
  const int N[3] = {g.nx, g.ny, g.nz};
  for (int ai = 0; ai < 3; ++ai) {
    const int a = e_side ? (ai + 1) % 3 : ai;
    PmlAxisDev& P = h->pml[a];
    if (P.n_lo + P.n_hi == 0 || !((axes >> a) & 1)) continue;
    const int c1 = (a + 1) % 3, c2 = (a + 2) % 3;
    // the two faces of an axis touch disjoint cells: ONE launch (blockIdx.y = face) — small and
    // mid-size grids are bound by the number of dependent launches, not by the slab work
    SlabP sl[2];
    long long cells[2] = {0, 0};
    int n_sl = 0;
    for (int side = 0; side < 2; ++side) {
      int s_lo, s_n, base;
      if (side == 0) { s_lo = 0; s_n = P.n_lo; base = 0; }
      else if (e_side) { s_lo = N[a] - P.n_hi + 1; s_n = P.n_hi - 1; base = P.lo + (s_lo - P.hi0); }
      else { s_lo = N[a] - P.n_hi; s_n = P.n_hi; base = P.lo + (s_lo - P.hi0); }
      if (s_n <= 0) continue;
      SlabP q;
      q.a = a; q.s_lo = s_lo; q.s_n = s_n; q.psi_base = base;
      q.psi_ns = P.ns;
      q.kbeg = kbeg; q.kend = kend; q.kpsi0 = 0;
      if (a == 2) {          // intersect the slab with the launch z-range
        int lo = s_lo > kbeg ? s_lo : kbeg;
        int hi = (s_lo + s_n) < kend ? (s_lo + s_n) : kend;
        if (hi <= lo) continue;
        q.kbeg = lo; q.kend = hi;
      }
      const long long bx = (a == 0) ? s_n : g.nx, by = (a == 1) ? s_n : g.ny;
      const long long total = bx * by * (q.kend - q.kbeg);
      if (total <= 0) continue;
      sl[n_sl] = q; cells[n_sl] = total; ++n_sl;
    }
    if (n_sl == 0) continue;
    if (n_sl == 1) sl[1] = sl[0];
    const bool vec4 = (a != 0) && (g.nx % 4 == 0);      // y / z slabs: float4 along x
    const long long most = std::max(cells[0], cells[1]);
    const dim3 grid(nblk(vec4 ? most / 4 : most), n_sl);
    if (e_side) {
      const auto kern = vec4 ? pml_slab_kernel<true, 4> : pml_slab_kernel<true, 1>;
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, g, sl[0], sl[1],
                         field_ptr(h, c1), field_ptr(h, c2), (const float*)field_ptr(h, 3 + c1), (const float*)field_ptr(h, 3 + c2),
                         P.psi_e[0], P.psi_e[1], (const float4*)P.ce4, SlabEP{h->idl[a], h->mat4, h->lut, h->cb1, h->mat4b});
    } else {
      const auto kern = vec4 ? pml_slab_kernel<false, 4> : pml_slab_kernel<false, 1>;
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, g, sl[0], sl[1],
                         field_ptr(h, 3 + c1), field_ptr(h, 3 + c2), (const float*)field_ptr(h, c1), (const float*)field_ptr(h, c2),
                         P.psi_h[0], P.psi_h[1], (const float4*)P.ch4, SlabHP{h->ip[a]});
    }
  }
}

// absorber layers over the planes [kbeg, kend): E components (end of the E phase) or H components
// (start of the H phase, before the H-side corrections).  One launch per axis and face.
void launch_damp(FdtdSolver* h, bool e_side, int kbeg, int kend, hipStream_t st) {
  dbg_sync(h);
  if (!h->has_damp || kend <= kbeg) return;
  const GridP& g = h->g;
  const int N[3] = {g.nx, g.ny, g.nz};
  DampP d;
  for (int a = 0; a < 3; ++a) {
    d.fb[a] = h->damp_fb[a]; d.fc[a] = h->damp_fc[a];
    d.lo[a] = h->damp_lo[a]; d.hi[a] = h->damp_hi[a];
  }
  const int off = e_side ? 0 : 3;
  float *f0 = field_ptr(h, off), *f1 = field_ptr(h, off + 1), *f2 = field_ptr(h, off + 2);
  for (int a = 0; a < 3; ++a)
    for (int side = 0; side < 2; ++side) {
      int s_lo = side == 0 ? 0 : h->damp_hi[a];
      int s_hi = side == 0 ? h->damp_lo[a] : N[a];
      if (a == 2) { s_lo = std::max(s_lo, kbeg); s_hi = std::min(s_hi, kend); }
      if (s_hi <= s_lo) continue;
      const long long bx = (a == 0) ? (s_hi - s_lo) : g.nx, by = (a == 1) ? (s_hi - s_lo) : g.ny;
      const long long bz = (a == 2) ? (s_hi - s_lo) : (kend - kbeg);
      const bool vec4 = a != 0 && g.nx % 4 == 0;        // y / z layers: float4 along x
      const auto kern = vec4 ? damp_kernel<4> : damp_kernel<1>;
      hipLaunchKernelGGL(kern, dim3(nblk((vec4 ? bx / 4 : bx) * by * bz)), dim3(256), 0, st,
                         g, d, f0, f1, f2, e_side ? 0 : 1, a, s_lo, s_hi - s_lo, kbeg, kend);
    }
}

// the lists of one side that inject at step n, in the order of for_each_source_side
void launch_sources(FdtdSolver* h, bool e_side, long long n, int kbeg, int kend, hipStream_t st, bool replica = false,
                    const FieldP* fs = nullptr) {
  dbg_sync(h);
  if (kend <= kbeg) return;
  const long long zlo = (long long)kbeg * h->g.sxy, zhi = (long long)kend * h->g.sxy;
  const int off = e_side ? 0 : 3;
  float *f0 = field_ptr(h, off), *f1 = field_ptr(h, off + 1), *f2 = field_ptr(h, off + 2);
  if (fs) { f0 = e_side ? fs->ex : fs->hx; f1 = e_side ? fs->ey : fs->hy; f2 = e_side ? fs->ez : fs->hz; }
  for (Tfsf& t : h->tfsf) {
    if (n >= t.n_steps) continue;
    const TfsfList& L = e_side ? t.e : t.h;
    // E-side corrections read the incident H (h1), H-side ones the incident E (e1)
    const float* aux = e_side ? (replica ? t.h1c : t.h1) : (replica ? t.e1c : t.e1);
    if (L.n && planes_meet(L.k0, L.k1, kbeg, kend))
      hipLaunchKernelGGL(tfsf_corr_kernel, dim3(nblk(L.n)), dim3(256), 0, st, f0, f1, f2,
                         (const int32_t*)L.comp, (const uint32_t*)L.cell, (const int32_t*)L.start, (const float*)L.w,
                         (const int32_t*)L.aux, aux, L.n, zlo, zhi);
  }
  for (PointSrc& s : h->psrc) {
    if (n >= s.n_steps) continue;
    const PointSide& P = s.side(e_side);
    if (P.n && planes_meet(P.k0, P.k1, kbeg, kend))
      hipLaunchKernelGGL(point_source_kernel, dim3(nblk(P.n)), dim3(256), 0, st, f0, f1, f2,
                         (const int32_t*)P.comp, (const uint32_t*)P.cell, (const float*)P.wre,
                         (const float*)P.wim, (const float2*)P.wave, h->step_dev_mode ? h->step_dev_off : n, P.n, zlo, zhi,
                         (const long long*)(h->step_dev_mode ? h->step_dev : nullptr));
  }
}

// the 1-D incident grids advance once per phase on the main stream (not z-range dependent)
void advance_tfsf_aux(FdtdSolver* h, bool e_side, long long n, hipStream_t st, bool replica = false) {
  dbg_sync(h);
  for (Tfsf& t : h->tfsf) {
    if (n >= t.n_steps) continue;
    float* e1 = replica ? t.e1c : t.e1;
    float* h1 = replica ? t.h1c : t.h1;
    if (e_side)
      hipLaunchKernelGGL(tfsf_aux_e_kernel, dim3(1), dim3(1024), 0, st, e1, (const float*)h1,
                         (const float*)t.ae, (const float*)t.be, t.n_aux, t.src_cell, (const float*)t.wave,
                         h->step_dev_mode ? h->step_dev_off : n, (const long long*)(h->step_dev_mode ? h->step_dev : nullptr));
    else
      hipLaunchKernelGGL(tfsf_aux_h_kernel, dim3(nblk(t.n_aux)), dim3(256), 0, st, h1, (const float*)e1,
                         (const float*)t.ah, (const float*)t.bh, t.n_aux);
  }
}

// fully anisotropic bodies: E^n of the neighbour nodes, saved in front of the E update ...
void aniso_save(FdtdSolver* h, hipStream_t st) {
  if (h->aniso.empty()) return;
  dbg_sync(h);
  for (AnisoGroup& a : h->aniso) {
    const float* b1 = field_ptr(h, (a.comp + 1) % 3);
    const float* b2 = field_ptr(h, (a.comp + 2) % 3);
    hipLaunchKernelGGL(aniso_save_kernel, dim3(nblk(8 * a.n)), dim3(256), 0, st, b1, b2, (const uint32_t*)a.nbr, a.old, 8 * a.n);
  }
}
// ... and the coupling, behind the E update and its sources: every component's correction from the unpatched values, then applied
void aniso_apply(FdtdSolver* h, hipStream_t st) {
  if (h->aniso.empty()) return;
  dbg_sync(h);
  for (AnisoGroup& a : h->aniso) {
    const float* b1 = field_ptr(h, (a.comp + 1) % 3);
    const float* b2 = field_ptr(h, (a.comp + 2) % 3);
    hipLaunchKernelGGL(aniso_delta_kernel, dim3(nblk(a.n)), dim3(256), 0, st, b1, b2, (const uint32_t*)a.nbr, (const float*)a.w_new,
                       (const float*)a.w_old, (const float*)a.old, a.delta, a.n);
  }
  for (AnisoGroup& a : h->aniso)
    hipLaunchKernelGGL(aniso_apply_kernel, dim3(nblk(a.n)), dim3(256), 0, st, field_ptr(h, a.comp), (const uint32_t*)a.cell,
                       (const float*)a.delta, a.n);
}

// the same two under Bloch boundaries (fdtd_run_bloch): the Re and Im handles carry the same lists; one launch per list saves E^n
// of both parts, one forms the deltas of both parts (slots across a Bloch face rotated by their wrap code's phase)
void aniso_save_bloch(FdtdSolver* hr, FdtdSolver* hi, hipStream_t st) {
  dbg_sync(hr);
  for (size_t k = 0; k < hr->aniso.size(); ++k) {
    AnisoGroup &ar = hr->aniso[k], &ai = hi->aniso[k];
    const int b1 = (ar.comp + 1) % 3, b2 = (ar.comp + 2) % 3;
    hipLaunchKernelGGL(aniso_save_bloch_kernel, dim3(nblk(8 * ar.n)), dim3(256), 0, st, (const float*)field_ptr(hr, b1),
                       (const float*)field_ptr(hr, b2), (const float*)field_ptr(hi, b1), (const float*)field_ptr(hi, b2),
                       (const uint32_t*)ar.nbr, ar.old, ai.old, 8 * ar.n);
  }
}
void aniso_apply_bloch(FdtdSolver* hr, FdtdSolver* hi, const AnisoPhaseTab& tab, hipStream_t st) {
  dbg_sync(hr);
  for (size_t k = 0; k < hr->aniso.size(); ++k) {
    AnisoGroup &ar = hr->aniso[k], &ai = hi->aniso[k];
    const int b1 = (ar.comp + 1) % 3, b2 = (ar.comp + 2) % 3;
    hipLaunchKernelGGL(aniso_delta_bloch_kernel, dim3(nblk(ar.n)), dim3(256), 0, st, (const float*)field_ptr(hr, b1),
                       (const float*)field_ptr(hr, b2), (const float*)field_ptr(hi, b1), (const float*)field_ptr(hi, b2),
                       (const uint32_t*)ar.nbr, (const uint8_t*)ar.wrap, (const float*)ar.w_new, (const float*)ar.w_old,
                       (const float*)ar.old, (const float*)ai.old, tab, ar.delta, ai.delta, ar.n);
  }
  for (FdtdSolver* h : {hr, hi})
    for (AnisoGroup& a : h->aniso)
      hipLaunchKernelGGL(aniso_apply_kernel, dim3(nblk(a.n)), dim3(256), 0, st, field_ptr(h, a.comp), (const uint32_t*)a.cell,
                         (const float*)a.delta, a.n);
}

// time-modulated media: E^n of the listed nodes, saved in front of the E update ...
void modulation_save(FdtdSolver* h, hipStream_t st) {
  if (h->modulation.empty()) return;
  dbg_sync(h);
  for (ModGroup& m : h->modulation)
    hipLaunchKernelGGL(modulation_save_kernel, dim3(nblk(m.n)), dim3(256), 0, st, (const float*)field_ptr(h, m.comp),
                       (const uint32_t*)m.cell, m.old, m.n);
}
// ... and the update with eps(t), sigma(t) in place of the table update, at the END of the E phase of step n (behind CPML, sources,
// damping and ADE; in front of the ghost fills).  The phases are formed in double from the step count: no drift over long runs.
void modulation_apply(FdtdSolver* h, long long n, hipStream_t st) {
  if (h->modulation.empty()) return;
  dbg_sync(h);
  for (ModGroup& m : h->modulation) {
    const double t0 = m.w_eps * (double)n, t1 = m.w_eps * (double)(n + 1), th = m.w_sig * ((double)n + 0.5);
    const ModPhase p{(float)std::cos(t0), (float)std::sin(t0), (float)std::cos(t1), (float)std::sin(t1), (float)std::cos(th),
                     (float)std::sin(th)};
    hipLaunchKernelGGL(modulation_apply_kernel, dim3(nblk(m.n)), dim3(256), 0, st, field_ptr(h, m.comp), (const uint32_t*)m.cell,
                       (const float*)m.ca, (const float*)m.eps_bar, (const float*)m.s_bar, (const float2*)m.d_eps,
                       (const float2*)m.d_s, (const float*)m.old, p, m.n);
  }
}

// Kerr media: E^n and I^n of the listed nodes, saved in front of the E update ...
NonlinearP nonlinear_args(FdtdSolver* h, long long* n_max) {
  NonlinearP p{};
  *n_max = 0;
  for (int c = 0; c < 3; ++c) p.e[c] = field_ptr(h, c);
  for (const NonlinearGroup& g : h->nonlinear) {
    p.l[g.comp] = NonlinearList{g.cell, g.nbr, g.den0, g.chi3, g.old, g.i_old, g.lin, g.next, g.n};
    *n_max = std::max(*n_max, g.n);
  }
  return p;
}
void nonlinear_save(FdtdSolver* h, hipStream_t st) {
  if (h->nonlinear.empty()) return;
  dbg_sync(h);
  long long n_max;
  const NonlinearP p = nonlinear_args(h, &n_max);
  hipLaunchKernelGGL(nonlinear_save_kernel, dim3(nblk(n_max), 3), dim3(256), 0, st, p);
}
// ... and the fixed-point iterations at the END of the E phase (behind CPML, sources, damping and ADE; in front of the ghost fills):
// per iteration every listed node of all three components is computed from the fields as the last iteration left them, then all
// are stored (Jacobi: no dependence on list or launch order)
void nonlinear_apply(FdtdSolver* h, hipStream_t st) {
  if (h->nonlinear.empty()) return;
  dbg_sync(h);
  long long n_max;
  const NonlinearP p = nonlinear_args(h, &n_max);
  const dim3 grid(nblk(n_max), 3);
  for (int m = 0; m < h->nonlinear_iters; ++m) {
    hipLaunchKernelGGL(nonlinear_iter_kernel, grid, dim3(256), 0, st, p, m == 0 ? 1 : 0);
    hipLaunchKernelGGL(nonlinear_scatter_kernel, grid, dim3(256), 0, st, p);
  }
}

// PEC-conformal boundaries: H of the cut faces gains what the conformal weights add to the sweep's own curl term (E^n alone)
void conformal_apply(FdtdSolver* h, hipStream_t st) {
  if (h->conformal.empty()) return;
  dbg_sync(h);
  for (ConformalGroup& c : h->conformal) {
    const int a = c.comp - 3;
    hipLaunchKernelGGL(conformal_h_kernel, dim3(nblk(c.n)), dim3(256), 0, st, field_ptr(h, c.comp), (const float*)field_ptr(h, (a + 2) % 3),
                       (const float*)field_ptr(h, (a + 1) % 3), (const uint32_t*)c.cell, (const uint32_t*)c.nbr, (const float*)c.d, c.n);
  }
}

void launch_ade(FdtdSolver* h, int kbeg, int kend, hipStream_t st, const FieldP* fs = nullptr) {
  dbg_sync(h);
  if (kend <= kbeg) return;
  const long long zlo = (long long)kbeg * h->g.sxy, zhi = (long long)kend * h->g.sxy;
  for (AdeGroup& a : h->ade) {
    if (!planes_meet(a.k0, a.k1, kbeg, kend)) continue;
    // a sorted list: the launch covers the entries of the planes [kbeg, kend) only — the boundary chunks of a z-slab step
    // (2 planes each, three launches per component and step) no longer scan the whole list three times
    long long t0 = 0, t1 = a.n;
    if (!a.plane_off.empty()) { t0 = a.plane_off[(size_t)std::max(kbeg, 0)]; t1 = a.plane_off[(size_t)std::min(kend, h->g.nz)]; }
    if (t1 <= t0) continue;
    float* ef = fs ? (a.comp == 0 ? fs->ex : (a.comp == 1 ? fs->ey : fs->ez)) : field_ptr(h, a.comp);
    const bool paged = h->disp.state == 1;      // (the memory term of the next step goes to the paged array the two-step sweeps read)
    hipLaunchKernelGGL(ade_kernel, dim3(nblk(t1 - t0)), dim3(256), 0, st, ef,
                       (const uint32_t*)a.cell + t0, a.e_old + t0, a.q + t0, t1 - t0, a.n, zlo, zhi, a.p,
                       paged ? h->disp.cs : nullptr, paged ? (const uint32_t*)a.qoff + t0 : nullptr);
  }
}

// ---- the terms around the field update of ONE SINGLE step, in the order that is part of the arithmetic -------------------------
// Every schedule that issues a single step (Run::fused_one, two_pass_step, tb_pair, the z-slab ranks' h_pre / e_post, BlochRun::step)
// calls these; the order is stated here and nowhere else.  (Step PAIRS — plain_pair, shell_pair, shell2_pair, slab_pair, middle_step —
// keep their own lists: what they launch depends on what their sweep has already applied.)  Each launcher returns without a launch
// when its list or layer count is empty, so a schedule that cannot carry a term (tb_pair: no CPML) launches nothing for it.
// `axes`: the CPML axes that run as slab kernels (7 & ~ the axes inside the sweep); `replica`: the comm stream's copy of the TFSF
// incident grids.  What stays with the caller, because its place differs between the schedules: fill_mirror, aniso_save /
// modulation_save / nonlinear_save, advance_tfsf_aux, the ghost fills, record_monitors.
// WHOLE-GRID LISTS (kListKind: the fully anisotropic, modulation, PEC-conformal and Kerr lists) are not sorted by plane, so a launch
// covers all their nodes or none: only a call that covers every plane applies them — h_side_terms with [0, nz), e_side_terms with
// `whole_grid` (Run::fused_one, Run::two_pass_step and BlochRun::step on one GPU).  A caller that works on a plane range (tb_pair's
// slabs, e_post and the cs / st halves of a z-slab rank) launches nothing for them: exactly the schedules whose set-up refuses the
// lists — refuse_lists_on_z_slabs (fdtd_add_*, fdtd_comm_init, Run::setup, BlochRun::setup) — or is not chosen with them: has_lists.
// H side, in FRONT of the update of step n, planes [k0, k1): absorber damping of H^{n-1/2}, then H-side sources / TFSF corrections
// (they only read E^n), then the CPML slabs — the summation order of the fused sweep — then the PEC-conformal correction of the cut
// faces (it reads E^n alone as well).
void h_side_terms(FdtdSolver* h, long long n, int k0, int k1, hipStream_t st, int axes = 7, bool replica = false) {
  launch_damp(h, false, k0, k1, st);
  launch_sources(h, false, n, k0, k1, st, replica);
  launch_pml(h, false, k0, k1, st, axes);
  if (k0 == 0 && k1 == h->g.nz) conformal_apply(h, st);
}
// E side, BEHIND the update of step n.  Head: the CPML slabs, then the E-side sources / TFSF corrections ...
void e_side_head(FdtdSolver* h, long long n, int k0, int k1, hipStream_t st, int axes = 7, bool replica = false) {
  launch_pml(h, true, k0, k1, st, axes);
  launch_sources(h, true, n, k0, k1, st, replica);
}
// ... tail: absorber damping, then the ADE pass (its stored E^{n+1} is the damped one), then the time-modulation patch (the end of
// the E phase: E_lin of the listed nodes is complete), then the Kerr media's fixed-point iterations (they read E_lin of all three
// components; a handle carries either kind of list, not both).  Between the two, the fully anisotropic coupling: aniso_apply, or
// aniso_apply_bloch where it reads both parts of a Bloch pair (BlochRun::step cuts in there).
// `whole_grid`: the call covers every plane of the grid (above).
void e_side_tail(FdtdSolver* h, long long n, int k0, int k1, hipStream_t st, bool whole_grid) {
  launch_damp(h, true, k0, k1, st);
  launch_ade(h, k0, k1, st);
  if (whole_grid) modulation_apply(h, n, st);
  if (whole_grid) nonlinear_apply(h, st);
}
void e_side_terms(FdtdSolver* h, long long n, int k0, int k1, hipStream_t st, bool whole_grid, int axes = 7, bool replica = false) {
  e_side_head(h, n, k0, k1, st, axes, replica);
  if (whole_grid) aniso_apply(h, st);
  e_side_tail(h, n, k0, k1, st, whole_grid);
}

// behind a two-step sweep that carried the ADE update of its first step (launch_fused2 with use_disp; set B = `fs` or the current
// set holds E^{n+2} with the sources and damping of step n + 1 applied): both steps of the pole states, E^{n+2} corrected
void launch_ade2(FdtdSolver* h, hipStream_t st, const FieldP* fs = nullptr) {
  dbg_sync(h);
  for (AdeGroup& a : h->ade) {
    float* ef = fs ? (a.comp == 0 ? fs->ex : (a.comp == 1 ? fs->ey : fs->ez)) : field_ptr(h, a.comp);
    hipLaunchKernelGGL(ade2_kernel, dim3(nblk(a.n)), dim3(256), 0, st, ef, (const uint32_t*)a.cell, a.e_old, a.q, a.n, a.p,
                       (const float*)h->disp.e1, h->disp.cs, (const uint32_t*)a.qoff);
  }
}

// One-off, before the first run that may take step pairs: the memory terms cc S(Q) of all dispersive cells go to PAGED storage
// (fdtd_fused2.hpp DispP) that the two-step sweeps address by position, and every ADE launch of the handle keeps them current from
// then on.  Needs sorted lists without repeats (one slot per entry), one GPU, packed medium words (the instantiations that carry
// the ADE lines are materials ones).  state = 1 (ready) or -1 (this problem keeps single steps / z holes as in round 5).
// -1 = a HIP error.
int disp_setup(FdtdSolver* h) {
  Disp& D = h->disp;
  if (D.state != 0) return 0;
  D.state = -1;
  const GridP& g = h->g;
  // (three kinds, not has_lists: Run::setup_pairs asks here whatever lists there are, and a handle with conformal lists has paged so far)
  if (h->ade.empty() || h->disp_on == 0 || !h->mat4 || h->mat4b || h->comm || !h->aniso.empty() || !h->modulation.empty() || !h->nonlinear.empty() || g.nx % 4 != 0) return 0;
  for (const AdeGroup& a : h->ade) if (!a.strict) return 0;
  const int nbx = (g.nx + 255) / 256;
  hipStream_t st = h->stream;
  auto give_up = [&]() { (void)hipGetLastError(); h->err.clear(); for (AdeGroup& a : h->ade) a.qoff = nullptr; return 0; };
  const int rc = seg_map_build(h, D.seg, [&](int* seg) {
    for (const AdeGroup& a : h->ade)
      hipLaunchKernelGGL(disp_mark_kernel, dim3(nblk(a.n)), dim3(256), 0, st, (const uint32_t*)a.cell, a.n, g.nx, nbx, seg);
  });
  if (rc) return rc < 0 ? -1 : give_up();             // (gives up past 2^32 floats: qoff is 32 bits wide)
  const size_t floats = (size_t)D.seg.n_blocks * 3 * 256;
  int* box = nullptr;
  if (dev_alloc(h, &D.cs, floats) || dev_alloc(h, &D.e1, floats) || box_seed_upload(h, &box)) return give_up();
  for (AdeGroup& a : h->ade) {
    if (dev_alloc(h, &a.qoff, (size_t)a.n, false)) return give_up();
    hipLaunchKernelGGL(disp_qoff_kernel, dim3(nblk(a.n)), dim3(256), 0, st, (const uint32_t*)a.cell, a.n, g.nx, g.ny, nbx,
                       (const int*)D.seg.dev, a.comp, (const float2*)a.q, a.p, a.qoff, D.cs, box);
  }
  int boxh[6];
  HIPCHK(h, hipMemcpyAsync(boxh, box, sizeof(boxh), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (int a = 0; a < 3; ++a) { D.lo[a] = boxh[2 * a]; D.hi[a] = boxh[2 * a + 1] + 1; }
  h->tile_cls.clear();
  h->box_paged.clear();
  D.state = 1;
  return 0;
}
// every dispersive cell `margin` cells (x: 4) or more inside the box [lo, hi) — a bulk the shell's boxes never recompute
bool disp_inside(const FdtdSolver* h, const int lo[3], const int hi[3], int margin) {
  const Disp& D = h->disp;
  if (D.state != 1) return false;
  for (int a = 0; a < 3; ++a) {
    const int m = a == 0 ? std::max(margin ? 8 : 4, margin) : margin;       // (x: whole float4 lanes; the boxes' halo lanes reach 8 columns)
    if (D.lo[a] < lo[a] + m || D.hi[a] > hi[a] - m) return false;
  }
  return true;
}

// One-off: slots for the nodes of every source list in paged storage (fdtd_fused2.hpp SrcP).  Needs one GPU and at most two LAYERS:
// a list goes to layer 0, or — where it meets an earlier list of its side (E / H) on a node: the second polarisation component of
// a TFSF box — to layer 1, which the kernels add behind layer 0 as the list kernels would one after the other; a list that meets a
// layer-1 list, or lists a node twice, leaves the problem to single steps.  state = 1 (ready) or -1.  -1 = a HIP error.
int spg_setup(FdtdSolver* h) {
  SrcPaged& S = h->spg;
  if (S.state != 0) return 0;
  S.state = -1;
  S.n_psrc = h->psrc.size(); S.n_tfsf = h->tfsf.size();
  const GridP& g = h->g;
  if (h->spg_on == 0 || h->comm || g.nx % 4 != 0) return 0;
  long long total = 0;
  for_each_source_side(h, [&](const auto& L, bool) { total += L.n; });
  if (total == 0) return 0;
  const int nbx = (g.nx + 255) / 256;
  hipStream_t st = h->stream;
  auto give_up = [&]() { (void)hipGetLastError(); h->err.clear(); return 0; };
  const int rc = seg_map_build(h, S.seg, [&](int* seg) {
    for_each_source_side(h, [&](const auto& L, bool) {
      hipLaunchKernelGGL(disp_mark_kernel, dim3(nblk(L.n)), dim3(256), 0, st, (const uint32_t*)L.cell, L.n, g.nx, nbx, seg);
    });
  });
  if (rc) return rc < 0 ? -1 : give_up();
  const size_t floats = (size_t)S.seg.n_blocks * 3 * 256;
  int *occ[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *box = nullptr, *hit = nullptr;       // [side][layer]
  if (dev_alloc(h, &S.e1, floats) || dev_alloc(h, &S.h2, floats) || dev_alloc(h, &S.e2, floats) || box_seed_upload(h, &box) ||
      dev_alloc(h, &hit, 2)) return give_up();
  for (int sd = 0; sd < 2; ++sd) for (int ly = 0; ly < 2; ++ly) if (dev_alloc(h, &occ[sd][ly], floats)) return give_up();
  bool failed = false, hip_failed = false;
  int layers = 1;
  S.any_h = false;
  for_each_source_side(h, [&](auto& L, bool h_side) {      // (in this order a list meets the lists added to the fields before it)
    if (failed || hip_failed) return;
    if (dev_alloc(h, &L.soff, (size_t)L.n, false)) { failed = true; return; }
    S.any_h = S.any_h || h_side;
    hipLaunchKernelGGL(src_soff_kernel, dim3(nblk(L.n)), dim3(256), 0, st, (const uint32_t*)L.cell, (const int32_t*)L.comp, L.n, g.nx, g.ny,
                       nbx, (const int*)S.seg.dev, L.soff, box);
    // the layer: above every earlier list of this side it meets
    int hh[2] = {0, 0};
    auto probe = [&](int ly, int mark) {
      if (hipMemsetAsync(hit, 0, 2 * sizeof(int), st) != hipSuccess) { hip_failed = true; return; }
      hipLaunchKernelGGL(src_layer_kernel, dim3(nblk(L.n)), dim3(256), 0, st, (const uint32_t*)L.soff, L.n, occ[h_side ? 1 : 0][ly], hit, mark);
      if (hipMemcpyAsync(hh, hit, sizeof(hh), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) hip_failed = true;
    };
    probe(1, 0);
    if (hip_failed) return;
    if (hh[0] > 0) { failed = true; return; }            // it would need a third layer
    probe(0, 0);
    if (hip_failed) return;
    L.layer = hh[0] > 0 ? 1 : 0;
    layers = std::max(layers, L.layer + 1);
    probe(L.layer, 1);
    if (!hip_failed && hh[1] > 0) failed = true;         // a node listed twice
  });
  for (int sd = 0; sd < 2; ++sd) for (int ly = 0; ly < 2; ++ly) release_buf(h, occ[sd][ly]);
  if (hip_failed) return fail(h, "spg_setup: a HIP call failed");
  if (failed) return give_up();
  if (layers > 1 && (dev_alloc(h, &S.e1b, floats) || dev_alloc(h, &S.h2b, floats) || dev_alloc(h, &S.e2b, floats)))
    return give_up();
  HIPCHK(h, hipStreamSynchronize(st));
  const SrcT tab{S.e1, S.h2, S.e2, S.any_h ? 1 : 0, 1, S.e1b, S.h2b, S.e2b};
  if (dev_upload(h, &S.tab, &tab, 1)) return give_up();
  S.state = 1;
  h->box_paged.clear();
  return 0;
}
// Lists were added (fdtd_add_point_source, fdtd_add_tfsf between two runs) since spg_setup laid the tables out — or gave up: the
// new list has no slots, a row segment of its own may have no block.  Everything goes back to "not tried" (the next setup_pairs
// builds it for the lists of now), with what was derived from the segment map: the tile classes, the boxes' flags.
void spg_release(FdtdSolver* h) {
  SrcPaged& S = h->spg;
  (void)hipStreamSynchronize(h->stream);
  auto drop = [&](auto*& p) { if (p) release_buf(h, p); p = nullptr; };
  drop(S.seg.dev); drop(S.e1); drop(S.h2); drop(S.e2); drop(S.e1b); drop(S.h2b); drop(S.e2b); drop(S.tab);
  for_each_source_side(h, [&](auto& L, bool) { drop(L.soff); L.layer = 0; });
  S.seg.host.clear();
  S.seg.n_blocks = 0; S.any_h = false;
  S.state = 0;
  h->tile_cls.clear();
  h->box_paged.clear();
}
// Shell2P::paged of a box: does a row segment it visits — rows j0 - 2 .. j1, planes k0 - 1 .. k1, columns i0 - 8 .. i1 + 7 — hold a
// source node (bit 0) / a dispersive cell (bit 1)?  Found once per box on the host maps of the segments.
int shell2_box_paged(FdtdSolver* h, const Shell2Box& bx) {
  const std::array<int, 6> key{bx.i0, bx.i1, bx.j0, bx.j1, bx.k0, bx.k1};
  auto it = h->box_paged.find(key);
  if (it != h->box_paged.end()) return it->second;
  const GridP& g = h->g;
  const int nbx = (g.nx + 255) / 256;
  const bool per_x = h->cfg.bc[0] == FDTD_BC_PERIODIC;
  const int t0 = per_x ? 0 : std::max(0, bx.i0 - 8) / 256, t1 = per_x ? nbx - 1 : std::min(g.nx - 1, bx.i1 + 7) / 256;
  int flags = 0;
  if (h->spg.state == 1 && h->spg.seg.any(g, bx.k0 - 1, bx.k1, bx.j0 - 2, bx.j1, t0, t1)) flags |= 1;
  if (h->disp.state == 1 && h->disp.seg.any(g, bx.k0 - 1, bx.k1, bx.j0 - 2, bx.j1, t0, t1)) flags |= 2;
  h->box_paged[key] = flags;
  return flags;
}
// the three arrays (per layer) of the pair (n, n + 1), and the incident grids of the TFSF boxes advanced through both steps: a side's lists
// as for_each_source_side orders them, the sides as two single steps do (the H-side terms of step n went into H^{n-1/2} just before, launch_sources):
//   incident H(n) | E-side terms of n | incident E(n) | H-side terms of n+1 | incident H(n+1) | E-side terms of n+1 | incident E(n+1)
void spg_fill(FdtdSolver* h, long long n, hipStream_t st) {
  SrcPaged& S = h->spg;
  auto fill = [&](float* val0, float* val1, bool e_side, long long step) {
    for (Tfsf& t : h->tfsf) {
      const TfsfList& L = e_side ? t.e : t.h;
      if (!L.n) continue;
      hipLaunchKernelGGL(src_fill_tfsf_kernel, dim3(nblk(L.n)), dim3(256), 0, st, L.layer ? val1 : val0, (const uint32_t*)L.soff,
                         (const int32_t*)L.start, (const float*)L.w, (const int32_t*)L.aux, (const float*)(e_side ? t.h1 : t.e1), L.n,
                         step >= t.n_steps ? 1 : 0);
    }
    for (PointSrc& s : h->psrc) {
      const PointSide& P = s.side(e_side);
      if (!P.n) continue;
      hipLaunchKernelGGL(src_fill_points_kernel, dim3(nblk(P.n)), dim3(256), 0, st, P.layer ? val1 : val0, (const uint32_t*)P.soff,
                         (const float*)P.wre, (const float*)P.wim, (const float2*)P.wave, step, P.n, step >= s.n_steps ? 1 : 0);
    }
  };
  advance_tfsf_aux(h, false, n, st, false);
  fill(S.e1, S.e1b, true, n);
  advance_tfsf_aux(h, true, n, st, false);
  if (S.any_h) fill(S.h2, S.h2b, false, n + 1);
  advance_tfsf_aux(h, false, n + 1, st, false);
  fill(S.e2, S.e2b, true, n + 1);
  advance_tfsf_aux(h, true, n + 1, st, false);
}
SrcP spg_params(const FdtdSolver* h) {
  const SrcPaged& S = h->spg;
  SrcP p;
  p.sseg = S.seg.dev; p.t = S.tab;
  return p;
}

// z boundary conditions of a single slab (no neighbour): fill ghost planes
void fill_ghost_h(FdtdSolver* h, hipStream_t st) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  const int bc0 = h->cfg.bc[4];
  if (bc0 == FDTD_BC_PERIODIC) {
    copy_plane(h, h->f.hx - pc, h->f.hx + (long long)(h->g.nz - 1) * pc, st);
    copy_plane(h, h->f.hy - pc, h->f.hy + (long long)(h->g.nz - 1) * pc, st);
  } else if (bc0 == FDTD_BC_PMC) {
    hipLaunchKernelGGL(negate_copy_kernel, dim3(nblk(pc)), dim3(256), 0, st, h->f.hx - pc, (const float*)h->f.hx, pc);
    hipLaunchKernelGGL(negate_copy_kernel, dim3(nblk(pc)), dim3(256), 0, st, h->f.hy - pc, (const float*)h->f.hy, pc);
  }
}
void fill_ghost_e(FdtdSolver* h, hipStream_t st) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  if (h->cfg.bc[5] == FDTD_BC_PERIODIC) {
    hipMemcpyAsync(h->f.ex + (long long)h->g.nz * pc, h->f.ex, pc * 4, hipMemcpyDeviceToDevice, st);
    hipMemcpyAsync(h->f.ey + (long long)h->g.nz * pc, h->f.ey, pc * 4, hipMemcpyDeviceToDevice, st);
  }
}

// ---- halo exchange over RCCL ----------------------------------------------------------------
// H phase: my top Hx,Hy plane -> upper neighbour's ghost(-1); E phase: my bottom Ex,Ey plane
// -> lower neighbour's ghost(nz).  Periodic z wraps rank n-1 <-> 0.
int exchange(FdtdSolver* h, bool e_side, hipStream_t st) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  const int nz = h->g.nz;
  const bool has_lo = h->cfg.bc[4] == FDTD_BC_NEIGHBOR, has_hi = h->cfg.bc[5] == FDTD_BC_NEIGHBOR;
  const int lo = (h->rank - 1 + h->n_ranks) % h->n_ranks, hi = (h->rank + 1) % h->n_ranks;
  NCCLCHK(h, ncclGroupStart());
  if (!e_side) {
    if (has_hi) {
      NCCLCHK(h, ncclSend(h->f.hx + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
      NCCLCHK(h, ncclSend(h->f.hy + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
    }
    if (has_lo) {
      NCCLCHK(h, ncclRecv(h->f.hx - pc, pc, ncclFloat, lo, h->comm, st));
      NCCLCHK(h, ncclRecv(h->f.hy - pc, pc, ncclFloat, lo, h->comm, st));
    }
  } else {
    if (has_lo) {
      NCCLCHK(h, ncclSend(h->f.ex, pc, ncclFloat, lo, h->comm, st));
      NCCLCHK(h, ncclSend(h->f.ey, pc, ncclFloat, lo, h->comm, st));
    }
    if (has_hi) {
      NCCLCHK(h, ncclRecv(h->f.ex + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
      NCCLCHK(h, ncclRecv(h->f.ey + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
    }
  }
  NCCLCHK(h, ncclGroupEnd());
  return 0;
}

// Fused sweep on z-slabs: the chunk prologue recomputes H^{n+1/2}[-1] from E^n[-1] (all three
// components) and the corrected H^{n-1/2}_{x,y}[-1]; the top plane needs E^n_{x,y}[nz].
//   exchange_fused_h : corrected H_x,H_y of my top plane  -> upper neighbour's ghost(-1)
//   exchange_fused_e : E_x,E_y,E_z of my top plane -> upper ghost(-1); E_x,E_y of my bottom plane
//                      -> lower neighbour's ghost(nz)
int exchange_fused_h(FdtdSolver* h, hipStream_t st) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  const int nz = h->g.nz;
  const bool has_lo = h->cfg.bc[4] == FDTD_BC_NEIGHBOR, has_hi = h->cfg.bc[5] == FDTD_BC_NEIGHBOR;
  const int lo = (h->rank - 1 + h->n_ranks) % h->n_ranks, hi = (h->rank + 1) % h->n_ranks;
  NCCLCHK(h, ncclGroupStart());
  if (has_hi) {
    NCCLCHK(h, ncclSend(h->f.hx + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
    NCCLCHK(h, ncclSend(h->f.hy + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
  }
  if (has_lo) {
    NCCLCHK(h, ncclRecv(h->f.hx - pc, pc, ncclFloat, lo, h->comm, st));
    NCCLCHK(h, ncclRecv(h->f.hy - pc, pc, ncclFloat, lo, h->comm, st));
  }
  NCCLCHK(h, ncclGroupEnd());
  return 0;
}

int exchange_fused_e(FdtdSolver* h, hipStream_t st) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  const int nz = h->g.nz;
  const bool has_lo = h->cfg.bc[4] == FDTD_BC_NEIGHBOR, has_hi = h->cfg.bc[5] == FDTD_BC_NEIGHBOR;
  const int lo = (h->rank - 1 + h->n_ranks) % h->n_ranks, hi = (h->rank + 1) % h->n_ranks;
  float* e3[3] = {h->f.ex, h->f.ey, h->f.ez};
  // RCCL pairs the k-th send to a peer with the k-th receive from it: when lo == hi (one or two
  // ranks, periodic z) the posting order below must mirror the peer's: [to-hi sends][to-lo sends]
  // on the sending side <-> [from-lo receives][from-hi receives] on the receiving side.
  NCCLCHK(h, ncclGroupStart());
  if (has_hi)
    for (float* p : e3) NCCLCHK(h, ncclSend(p + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
  if (has_lo) {
    NCCLCHK(h, ncclSend(h->f.ex, pc, ncclFloat, lo, h->comm, st));
    NCCLCHK(h, ncclSend(h->f.ey, pc, ncclFloat, lo, h->comm, st));
    for (float* p : e3) NCCLCHK(h, ncclRecv(p - pc, pc, ncclFloat, lo, h->comm, st));
  }
  if (has_hi) {
    NCCLCHK(h, ncclRecv(h->f.ex + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
    NCCLCHK(h, ncclRecv(h->f.ey + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
  }
  NCCLCHK(h, ncclGroupEnd());
  return 0;
}

// Pipelined z-slab schedule: ONE exchange per step carries everything the neighbours' boundary
// chunks need for the next sweep — up: E_x,E_y,E_z and the pre-corrected H_x,H_y of my top plane
// (-> upper ghost(-1)); down: E_x,E_y of my bottom plane (-> lower ghost(nz)).
// `fs`: the set whose planes travel (default: the current one) — the middle step of a slab pair ships the third set's.
// psi_set: which H-side psi arrays travel (the sender's newest top plane -> slot nz of the set the receiver's next sweep reads):
// 0 = the current set, 1 = the temporary set of a z hole (after the first step of a CPML slab pair), 2 = the other set of the
// ping-pong (after its second step, before the swap)
int exchange_fused_all(FdtdSolver* h, hipStream_t st, bool pml_with_sweep = false, const FieldP* fs = nullptr, int psi_set = 0) {
  dbg_sync(h);
  const long long pc = plane_cells(h);
  const int nz = h->g.nz;
  const bool has_lo = h->cfg.bc[4] == FDTD_BC_NEIGHBOR, has_hi = h->cfg.bc[5] == FDTD_BC_NEIGHBOR;
  if (!has_lo && !has_hi) return 0;
  const int lo = (h->rank - 1 + h->n_ranks) % h->n_ranks, hi = (h->rank + 1) % h->n_ranks;
  const FieldP F = fs ? *fs : h->f;
  float* up5[5] = {F.ex, F.ey, F.ez, F.hx, F.hy};
  // With the x / y CPML inside the sweep the chunk prologue of the upper rank corrects H[-1] itself and needs the
  // H-side psi of that plane — my top plane, CURRENT set (what the next sweep reads): into slot nz of its arrays.
  // Decided by the configuration alone (both sides must post the same messages), not by what a rank's sweep ends up doing.
  const bool psi_too = pml_with_sweep && h->pml_fused > 0;
  auto psi_of = [&](int a, int q) { return h->pml[a].set(psi_set == 1 ? PmlAxisDev::kHt : (psi_set == 2 ? PmlAxisDev::kH2 : PmlAxisDev::kH))[q]; };
  // posting order mirrors the peer's (see exchange_fused_e): [to-hi][to-lo] <-> [from-lo][from-hi]
  NCCLCHK(h, ncclGroupStart());
  if (has_hi) {
    for (float* p : up5) NCCLCHK(h, ncclSend(p + (long long)(nz - 1) * pc, pc, ncclFloat, hi, h->comm, st));
    if (psi_too)
      for (int a = 0; a < 2; ++a)
        for (int q = 0; q < 2 && h->pml[a].ns > 0; ++q)
          NCCLCHK(h, ncclSend(psi_of(a, q) + (size_t)(nz - 1) * h->pml[a].psi_plane, h->pml[a].psi_plane, ncclFloat, hi, h->comm, st));
  }
  if (has_lo) {
    NCCLCHK(h, ncclSend(F.ex, pc, ncclFloat, lo, h->comm, st));
    NCCLCHK(h, ncclSend(F.ey, pc, ncclFloat, lo, h->comm, st));
    for (float* p : up5) NCCLCHK(h, ncclRecv(p - pc, pc, ncclFloat, lo, h->comm, st));
    if (psi_too)
      for (int a = 0; a < 2; ++a)
        for (int q = 0; q < 2 && h->pml[a].ns > 0; ++q)
          NCCLCHK(h, ncclRecv(psi_of(a, q) + (size_t)nz * h->pml[a].psi_plane, h->pml[a].psi_plane, ncclFloat, lo, h->comm, st));
  }
  if (has_hi) {
    NCCLCHK(h, ncclRecv(F.ex + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
    NCCLCHK(h, ncclRecv(F.ey + (long long)nz * pc, pc, ncclFloat, hi, h->comm, st));
  }
  NCCLCHK(h, ncclGroupEnd());
  return 0;
}

// ---- field energy (K7) ------------------------------------------------------------------------
// W = sum |E|^2 + eta0^2 sum |H|^2 over the slab: fixed launch geometry, two passes, no atomics
int eval_energy(FdtdSolver* h, hipStream_t st, double* out) {
  const long long nc = n_cells(h);
  unsigned blocks = nblk(nc);
  if (blocks > (unsigned)kEnergyBlocks) blocks = kEnergyBlocks;
  hipLaunchKernelGGL(energy_partial_kernel, dim3(blocks), dim3(256), 0, st, (const float*)h->f.ex, (const float*)h->f.ey,
                     (const float*)h->f.ez, (const float*)h->f.hx, (const float*)h->f.hy, (const float*)h->f.hz, nc,
                     h->energy_dev + 1);
  hipLaunchKernelGGL(energy_final_kernel, dim3(1), dim3(256), 0, st, (const double*)(h->energy_dev + 1), (int)blocks,
                     h->energy_dev);
  HIPCHK(h, hipMemcpyAsync(out, h->energy_dev, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return 0;
}

// ---- monitors ---------------------------------------------------------------------------------
void record_monitors(FdtdSolver* h, long long n, bool post, hipStream_t st, const F2Plan* in_sweep = nullptr) {
  dbg_sync(h);
  for (size_t mi = 0; mi < h->mons.size(); ++mi) {
    Monitor& m = h->mons[mi];
    if (m.next >= m.steps.size() || m.steps[m.next] != n) continue;
    if (in_sweep) {                    // monitors recorded behind the two-step sweep (pair_record)
      bool skip = false;
      for (int q : in_sweep->mons) skip = skip || q == (int)mi;
      if (skip) continue;
    }
    const long long rec = (long long)m.next;
    const int nc = (int)m.comps.size();
    // one launch per monitor and phase.  pre (before the H update): E^n, and half of H^{n-1/2} for
    // time monitors; post (after it): the other half of H / the H terms of the running DFT.
    RecP r{};
    for (int ic = 0; ic < nc; ++ic) {
      const int c = m.comps[ic];
      const bool is_h = c >= 3;
      bool take;
      if (m.kind == FDTD_MON_TIME) take = is_h || !post;
      else take = is_h == post;
      if (!take) continue;
      r.f[r.n] = field_ptr(h, c);
      r.slot[r.n] = ic;
      r.scale[r.n] = is_h ? 0.5f : 1.0f;
      r.acc[r.n] = is_h ? 1 : 0;
      r.n++;
    }
    if (r.n > 0 && m.cells > 0) {
      const dim3 grid(nblk(m.cells), r.n);
      if (m.kind == FDTD_MON_TIME) {
        if (has_ring(m) && (size_t)rec - m.reduced >= m.ring) ring_drain(h, st);      // (a full ring: its complete records first)
        float* out = reinterpret_cast<float*>(m.data) + m.slot((size_t)rec) * nc * m.cells;
        hipLaunchKernelGGL(time_record_multi_kernel, grid, dim3(256), 0, st, r, h->g, m.box, out, (long long)m.cells);
      } else if (m.form == MonForm::SparseDft || m.form == MonForm::LatticeDft) {      // the live fields at the box origin
        FieldDftSrc s{};
        s.n = r.n; s.sy = h->g.nx; s.sz = h->g.sxy;
        for (int q = 0; q < r.n; ++q) {
          s.slot[q] = r.slot[q];
          s.f[q] = r.f[q] + (long long)m.box.lo2 * h->g.sxy + (long long)m.box.lo1 * h->g.nx + m.box.lo0;
        }
        launch_field_dft(h, m, s, (const float2*)((post ? m.phase_h : m.phase_e) + rec * m.nf), st);
      } else {
        const long long fstride = (long long)nc * m.cells;
        hipLaunchKernelGGL(dft_record_multi_kernel, grid, dim3(256), 0, st, r, h->g, m.box,
                           reinterpret_cast<float2*>(m.data), (long long)m.cells, fstride,
                           (const float2*)((post ? m.phase_h : m.phase_e) + rec * m.nf), m.nf);
      }
    }
    if (post) m.next++;
  }
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* fdtd_last_error(const FdtdSolver* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fdtd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fdtd_far_field(int device, int n_u, int n_v, const double* u, const double* v, const double* wu, const double* wv,
                   const double* currents, double w0, double k_re, double k_im, int n_dir, const double* r_u,
                   const double* r_v, const double* r_w, double* out) {
  if (n_u < 1 || n_v < 1 || n_dir < 0 || !u || !v || !wu || !wv || !currents || (n_dir && (!r_u || !r_v || !r_w || !out)))
    return fail(nullptr, "fdtd_far_field: bad argument");
  if (n_dir == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, "fdtd_far_field: hipSetDevice(%d) failed", device);
  const size_t n = (size_t)n_u * n_v;
  const size_t sizes[9] = {(size_t)n_u, (size_t)n_v, (size_t)n_u, (size_t)n_v, 8 * n, (size_t)n_dir, (size_t)n_dir,
                           (size_t)n_dir, 8 * (size_t)n_dir};
  const double* host[8] = {u, v, wu, wv, currents, r_u, r_v, r_w};
  double* dev[9] = {};
  int rc = 0;
  for (int i = 0; i < 9 && !rc; ++i) {
    if (hipMalloc((void**)&dev[i], sizes[i] * sizeof(double)) != hipSuccess) rc = fail(nullptr, "fdtd_far_field: out of device memory");
    else if (i < 8 && hipMemcpy(dev[i], host[i], sizes[i] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(nullptr, "fdtd_far_field: upload failed");
  }
  if (!rc) {
    FarP p;
    p.u = dev[0]; p.v = dev[1]; p.wu = dev[2]; p.wv = dev[3];
    p.cur = reinterpret_cast<const double2*>(dev[4]);
    p.n_u = n_u; p.n_v = n_v; p.w0 = w0; p.k_re = k_re; p.k_im = k_im;
    p.r_u = dev[5]; p.r_v = dev[6]; p.r_w = dev[7]; p.out = dev[8];
    hipLaunchKernelGGL(far_field_kernel, dim3((unsigned)n_dir), dim3(256), 0, 0, p);
    if (hipMemcpy(out, dev[8], sizes[8] * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(nullptr, "fdtd_far_field: %s", hipGetErrorString(hipGetLastError()));
  }
  for (double* q : dev) if (q) hipFree(q);
  return rc;
}

int fdtd_near_field_chunks(int n_pts, int n_u, int n_v) {
  if (n_pts < 0 || n_u < 1 || n_v < 1 || (long long)n_u * n_v > 0x7fffffffLL) return fail(nullptr, "fdtd_near_field_chunks: bad argument");
  return near_field_chunks(n_pts, (long long)n_u * n_v).chunks;
}

int fdtd_near_field(int device, int n_u, int n_v, const double* u, const double* v, const double* wu, const double* wv,
                    const double* currents, double w0, double k_re, double k_im, int n_pts, const double* p_u,
                    const double* p_v, const double* p_w, double* out) {
  if (n_u < 1 || n_v < 1 || n_pts < 0 || !u || !v || !wu || !wv || !currents || (n_pts && (!p_u || !p_v || !p_w || !out)))
    return fail(nullptr, "fdtd_near_field: bad argument");
  if ((long long)n_u * n_v > 0x7fffffffLL) return fail(nullptr, "fdtd_near_field: lattice of %d x %d nodes exceeds the 2^31 node index range", n_u, n_v);
  if (n_pts == 0) return 0;
  const size_t n = (size_t)n_u * n_v;
  const NearChunks ch = near_field_chunks(n_pts, (long long)n);
  if ((long long)n_pts * ch.chunks > 0x7fffffffLL) return fail(nullptr, "fdtd_near_field: too many points (%d)", n_pts);
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, "fdtd_near_field: hipSetDevice(%d) failed", device);
  // the partial records exist only where the lattice is cut (fdtd_near_field.hpp: at most 8184 of them)
  const size_t sizes[10] = {(size_t)n_u, (size_t)n_v, (size_t)n_u, (size_t)n_v, 8 * n, (size_t)n_pts, (size_t)n_pts,
                            (size_t)n_pts, 24 * (size_t)n_pts, ch.chunks > 1 ? 24 * (size_t)n_pts * ch.chunks : 0};
  const double* host[8] = {u, v, wu, wv, currents, p_u, p_v, p_w};
  double* dev[10] = {};
  int rc = 0;
  for (int i = 0; i < 10 && !rc; ++i) {
    if (!sizes[i]) continue;
    if (hipMalloc((void**)&dev[i], sizes[i] * sizeof(double)) != hipSuccess) rc = fail(nullptr, "fdtd_near_field: out of device memory");
    else if (i < 8 && hipMemcpy(dev[i], host[i], sizes[i] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(nullptr, "fdtd_near_field: upload failed");
  }
  if (!rc) {
    NearP p;
    p.u = dev[0]; p.v = dev[1]; p.wu = dev[2]; p.wv = dev[3];
    p.cur = reinterpret_cast<const double2*>(dev[4]);
    p.n_u = n_u; p.n_v = n_v; p.w0 = w0; p.k_re = k_re; p.k_im = k_im;
    p.p_u = dev[5]; p.p_v = dev[6]; p.p_w = dev[7];
    p.chunks = ch.chunks; p.chunk_len = ch.chunk_len;
    p.dst = ch.chunks > 1 ? dev[9] : dev[8];
    hipLaunchKernelGGL(near_field_kernel, dim3((unsigned)((long long)n_pts * ch.chunks)), dim3(256), 0, 0, p);
    if (ch.chunks > 1) {
      const long long n_vals = 24LL * n_pts;
      hipLaunchKernelGGL(near_field_sum_kernel, dim3((unsigned)((n_vals + 255) / 256)), dim3(256), 0, 0, (const double*)dev[9], dev[8],
                         ch.chunks, n_vals);
    }
    if (hipMemcpy(out, dev[8], sizes[8] * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(nullptr, "fdtd_near_field: %s", hipGetErrorString(hipGetLastError()));
  }
  for (double* q : dev) if (q) hipFree(q);
  return rc;
}

int fdtd_rasterize(const FdtdRasterJob* job, uint16_t* out_host) {
  if (!job || !out_host) return fail(nullptr, "fdtd_rasterize: null argument");
  if (job->struct_bytes != (int)sizeof(FdtdRasterJob) || job->record_bytes != (int)sizeof(FdtdRasterRecord))
    return fail(nullptr, "fdtd_rasterize: job of %d bytes with records of %d: this library has %d and %d", job->struct_bytes,
                job->record_bytes, (int)sizeof(FdtdRasterJob), (int)sizeof(FdtdRasterRecord));
  if (!job->records) return fail(nullptr, "fdtd_rasterize: null argument");
  for (int q = 0; q < 9; ++q)
    if (!job->coords[q]) return fail(nullptr, "fdtd_rasterize: null argument");
  if (job->n == 0) return fail(nullptr, "fdtd_rasterize: no records (n == 0)");
  const int shape[3] = {job->nx, job->ny, job->nz};
  if (job->n < 0 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || (long long)shape[0] * shape[1] * shape[2] >= (1LL << 32))
    return fail(nullptr, "fdtd_rasterize: bad grid %d x %d x %d or record count %lld", shape[0], shape[1], shape[2], (long long)job->n);
  long long launches = 0;
  for (int64_t r = 0; r < job->n; ++r) {
    const FdtdRasterRecord& rec = job->records[r];
    if (rec.kind != FDTD_RASTER_BOX && rec.kind != FDTD_RASTER_SPHERE && rec.kind != FDTD_RASTER_CYLINDER)
      return fail(nullptr, "fdtd_rasterize: record %lld: unknown kind %d", (long long)r, rec.kind);
    if (rec.kind == FDTD_RASTER_CYLINDER && (rec.axis < 0 || rec.axis > 2))
      return fail(nullptr, "fdtd_rasterize: record %lld: bad cylinder axis %d", (long long)r, rec.axis);
    for (int c = 0; c < 3; ++c) {
      if (rec.medium[c] < 0 || rec.medium[c] > 0xffff)
        return fail(nullptr, "fdtd_rasterize: record %lld: medium index %d is no uint16", (long long)r, rec.medium[c]);
      bool empty = false;
      for (int a = 0; a < 3; ++a) {
        if (rec.lo[c][a] < 0 || rec.hi[c][a] > shape[a])
          return fail(nullptr, "fdtd_rasterize: record %lld, component %d: index box [%d, %d) along axis %d outside the shape (%d nodes)",
                      (long long)r, c, rec.lo[c][a], rec.hi[c][a], a, shape[a]);
        empty = empty || rec.lo[c][a] >= rec.hi[c][a];
      }
      if (!empty) ++launches;
    }
  }
  // (grid.y = ceil(by / 4) and grid.z = bz of a launch are at most 65535: the node counts along y and z bound them)
  if (shape[1] > 4 * 65535 || shape[2] > 65535)
    return fail(nullptr, "fdtd_rasterize: %d x %d nodes along y, z exceed the launch grid", shape[1], shape[2]);
  if (hipSetDevice(job->device) != hipSuccess) return fail(nullptr, "fdtd_rasterize: hipSetDevice(%d) failed", job->device);
  const size_t cells = (size_t)shape[0] * shape[1] * shape[2], count = 3 * cells, n16 = (count + 7) / 8;
  size_t off[10] = {0};
  for (int q = 0; q < 9; ++q) off[q + 1] = off[q] + (size_t)shape[q % 3];
  double* d_coords = nullptr;
  uint4* d_out = nullptr;
  hipStream_t st = nullptr;
  int rc = 0;
  if (hipMalloc((void**)&d_coords, off[9] * sizeof(double)) != hipSuccess || hipMalloc((void**)&d_out, n16 * sizeof(uint4)) != hipSuccess)
    rc = fail(nullptr, "fdtd_rasterize: out of device memory (%zu bytes)", n16 * sizeof(uint4));
  if (!rc && hipStreamCreate(&st) != hipSuccess) rc = fail(nullptr, "fdtd_rasterize: hipStreamCreate failed");
  for (int q = 0; q < 9 && !rc; ++q)
    if (hipMemcpyAsync(d_coords + off[q], job->coords[q], (size_t)shape[q % 3] * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
      rc = fail(nullptr, "fdtd_rasterize: upload failed");
  if (!rc) {
    const unsigned blocks = (unsigned)std::min<size_t>((n16 + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(raster_fill_kernel, dim3(blocks), dim3(256), 0, st, d_out, (long long)n16, 1u);
    for (int64_t r = 0; r < job->n; ++r) {
      const FdtdRasterRecord& rec = job->records[r];
      for (int c = 0; c < 3; ++c) {
        RasterP p;
        p.xs = d_coords + off[3 * c]; p.ys = d_coords + off[3 * c + 1]; p.zs = d_coords + off[3 * c + 2];
        p.out = reinterpret_cast<unsigned short*>(d_out) + (size_t)c * cells;
        p.nx = shape[0]; p.ny = shape[1];
        p.lo0 = rec.lo[c][0]; p.lo1 = rec.lo[c][1]; p.lo2 = rec.lo[c][2];
        p.hi0 = rec.hi[c][0]; p.hi1 = rec.hi[c][1]; p.hi2 = rec.hi[c][2];
        if (p.lo0 >= p.hi0 || p.lo1 >= p.hi1 || p.lo2 >= p.hi2) continue;
        p.c0 = rec.center[0]; p.c1 = rec.center[1]; p.c2 = rec.center[2];
        p.s0 = rec.size[0]; p.s1 = rec.size[1]; p.s2 = rec.size[2];
        p.axis = rec.axis;
        p.medium = (unsigned short)rec.medium[c];
        const dim3 grid((unsigned)((p.hi0 - p.lo0 + kRasterLanes - 1) / kRasterLanes),
                        (unsigned)((p.hi1 - p.lo1 + kRasterRows - 1) / kRasterRows), (unsigned)(p.hi2 - p.lo2));
        const dim3 block(kRasterLanes, kRasterRows);
        if (rec.kind == FDTD_RASTER_BOX) hipLaunchKernelGGL(raster_paint_kernel<kRasterBox>, grid, block, 0, st, p);
        else if (rec.kind == FDTD_RASTER_SPHERE) hipLaunchKernelGGL(raster_paint_kernel<kRasterSphere>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(raster_paint_kernel<kRasterCylinder>, grid, block, 0, st, p);
      }
    }
    if (hipMemcpyAsync(out_host, d_out, count * sizeof(uint16_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      rc = fail(nullptr, "fdtd_rasterize: %s", hipGetErrorString(hipGetLastError()));
  }
  if (st) hipStreamDestroy(st);
  if (d_coords) hipFree(d_coords);
  if (d_out) hipFree(d_out);
  return rc;
}

int fdtd_create(const FdtdConfig* cfg, FdtdSolver** out) {
  if (!cfg || !out) return fail(nullptr, "fdtd_create: null argument");
  if (cfg->nx < 1 || cfg->ny < 1 || cfg->nz < 1) return fail(nullptr, "fdtd_create: bad grid %d x %d x %d", cfg->nx, cfg->ny, cfg->nz);
  if ((long long)cfg->nx * cfg->ny * (cfg->nz + 2) >= (1LL << 32))
    return fail(nullptr, "fdtd_create: slab of %d x %d x %d cells exceeds the 2^32 cell index range", cfg->nx, cfg->ny, cfg->nz);
  for (int a = 0; a < 3; ++a) {
    const bool p0 = cfg->bc[2 * a] == FDTD_BC_PERIODIC, p1 = cfg->bc[2 * a + 1] == FDTD_BC_PERIODIC;
    if (p0 != p1 && a < 2) return fail(nullptr, "fdtd_create: periodic boundary must be set on both faces of axis %d", a);
    if (cfg->bc[2 * a + 1] == FDTD_BC_PMC) return fail(nullptr, "fdtd_create: PMC is supported on min faces only");
    if (a < 2 && (cfg->bc[2 * a] == FDTD_BC_NEIGHBOR || cfg->bc[2 * a + 1] == FDTD_BC_NEIGHBOR))
      return fail(nullptr, "fdtd_create: neighbour faces exist only along z");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "fdtd_create: no HIP device available");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "fdtd_create: device %d out of range (%d devices)", cfg->device, ndev);
  FdtdSolver* h = new FdtdSolver();
  h->cfg = *cfg;
  h->no_jlo = getenv("FDTD_NO_JLO") != nullptr;
  if (hipSetDevice(cfg->device) != hipSuccess) { delete h; return fail(nullptr, "hipSetDevice(%d) failed", cfg->device); }
  GridP& g = h->g;
  g.nx = cfg->nx; g.ny = cfg->ny; g.nz = cfg->nz;
  g.sxy = (long long)cfg->nx * cfg->ny;
  g.bcx0 = cfg->bc[0]; g.bcx1 = cfg->bc[1]; g.bcy0 = cfg->bc[2]; g.bcy1 = cfg->bc[3];
  g.pec_z0 = cfg->bc[4] == FDTD_BC_PEC;
  g.psi_ghost = cfg->bc[4] == FDTD_BC_NEIGHBOR ? 1 : 0;
  g.ch = cfg->ch;
  // measured on MI355X, 512^3 (profiles/r01a_probe_geometry_512.jsonl): short z-marches win —
  // the 256 MiB Infinity Cache already serves the k+1 plane re-read, and more, smaller
  // workgroups balance the 256 CUs better than long marches.
  h->zchunk = cfg->z_chunk > 0 ? cfg->z_chunk : 2;
  h->zchunk_f = cfg->z_chunk > 0 ? cfg->z_chunk : 16;
  h->user_geometry = cfg->z_chunk > 0;
  h->rows = 4;
  int rc = 0;
  const size_t fcount = (size_t)g.sxy * (g.nz + 2);
  h->field_bytes = fcount * sizeof(float);
  rc = alloc_field_set(h, h->fbase, fcount, 0);
  if (!rc) {
    h->f.ex = h->fbase[0] + g.sxy; h->f.ey = h->fbase[1] + g.sxy; h->f.ez = h->fbase[2] + g.sxy;
    h->f.hx = h->fbase[3] + g.sxy; h->f.hy = h->fbase[4] + g.sxy; h->f.hz = h->fbase[5] + g.sxy;
    rc = dev_alloc(h, &h->energy_dev, 1 + kEnergyBlocks);
  }
  if (!rc) {
    // default: unit steps, vacuum
    const int N[3] = {g.nx, g.ny, g.nz};
    for (int a = 0; a < 3 && !rc; ++a) {
      // the z vectors carry one ghost entry below and above (indices -1 and nz)
      std::vector<float> ones(N[a] + (a == 2 ? 2 : 0), 1.0f);
      rc = dev_upload(h, &h->ip[a], (const float*)ones.data(), ones.size());
      if (!rc) rc = dev_upload(h, &h->idl[a], (const float*)ones.data(), ones.size());
      if (!rc && a == 2) {
        h->step_base[0] = h->ip[2]; h->step_base[1] = h->idl[2];
        h->ip[2] += 1; h->idl[2] += 1;
      }
    }
  }
  if (!rc && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(nullptr, "hipStreamCreate failed");
  // The comm stream carries the ghost exchanges and the boundary chunks.  High priority: its few
  // workgroups are dispatched ahead of the interior sweep's, otherwise the RCCL Send/Recv kernel
  // queues behind a full machine (measured: 138 us instead of 30 us, profiles/r01h_slab_timeline.txt).
  if (!rc) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
    if (hipStreamCreateWithPriority(&h->comm_stream, hipStreamNonBlocking, greatest) != hipSuccess)
      rc = fail(nullptr, "hipStreamCreate failed");
  }
  if (!rc) {
    hipEventCreate(&h->ev0); hipEventCreate(&h->ev1);
    hipEventCreateWithFlags(&h->ev_h_int, hipEventDisableTiming);
    hipEventCreateWithFlags(&h->ev_h_bnd, hipEventDisableTiming);
    hipEventCreateWithFlags(&h->ev_e_int, hipEventDisableTiming);
    hipEventCreateWithFlags(&h->ev_e_bnd, hipEventDisableTiming);
  }
  if (rc) {
    g_create_error = h->err.empty() ? g_create_error : h->err;
    fdtd_destroy(h);
    return -1;
  }
  *out = h;
  return 0;
}

void fdtd_destroy(FdtdSolver* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  hipDeviceSynchronize();
  if (h->comm) ncclCommDestroy(h->comm);
  for (DevBuf& b : h->bufs) hipFree(b.p);
  for (hipEvent_t e : h->kev) hipEventDestroy(e);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->ev_h_int) hipEventDestroy(h->ev_h_int);
  if (h->ev_h_bnd) hipEventDestroy(h->ev_h_bnd);
  if (h->ev_e_int) hipEventDestroy(h->ev_e_int);
  if (h->ev_e_bnd) hipEventDestroy(h->ev_e_bnd);
  if (h->ev_shell_a) hipEventDestroy(h->ev_shell_a);
  if (h->ev_rec) hipEventDestroy(h->ev_rec);
  if (h->ev_shell_b) hipEventDestroy(h->ev_shell_b);
  if (h->stream) hipStreamDestroy(h->stream);
  if (h->comm_stream && !h->streams_shared) hipStreamDestroy(h->comm_stream);
  if (h->box_stream) hipStreamDestroy(h->box_stream);
  if (h->ev_box) hipEventDestroy(h->ev_box);
  if (h->ev_box_in) hipEventDestroy(h->ev_box_in);
  delete h;
}

int fdtd_set_steps(FdtdSolver* h, int axis, const float* inv_primal, const float* inv_dual, int n) {
  if (!h) return -1;
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  if (axis < 0 || axis > 2) return fail(h, "fdtd_set_steps: bad axis %d", axis);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (axis == 2 && n == N[2] + 2) {        // ghost entries supplied (z-slab of a non-uniform grid)
    HIPCHK(h, hipMemcpy(h->step_base[0], inv_primal, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->step_base[1], inv_dual, (size_t)n * 4, hipMemcpyHostToDevice));
    return 0;
  }
  if (n != N[axis]) return fail(h, "fdtd_set_steps: axis %d expects %d entries, got %d", axis, N[axis], n);
  HIPCHK(h, hipMemcpy(h->ip[axis], inv_primal, (size_t)n * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->idl[axis], inv_dual, (size_t)n * 4, hipMemcpyHostToDevice));
  if (axis == 2) {                         // ghost entries: wrap for periodic z, replicate otherwise
    const bool per = h->cfg.bc[4] == FDTD_BC_PERIODIC;
    const float lo[2] = {per ? inv_primal[n - 1] : inv_primal[0], per ? inv_dual[n - 1] : inv_dual[0]};
    const float hi[2] = {per ? inv_primal[0] : inv_primal[n - 1], per ? inv_dual[0] : inv_dual[n - 1]};
    for (int q = 0; q < 2; ++q) {
      HIPCHK(h, hipMemcpy(h->step_base[q], &lo[q], 4, hipMemcpyHostToDevice));
      HIPCHK(h, hipMemcpy(h->step_base[q] + n + 1, &hi[q], 4, hipMemcpyHostToDevice));
    }
  }
  return 0;
}

int fdtd_set_media(FdtdSolver* h, const float* ca, const float* cb, int n_media) {
  if (!h) return -1;
  if (n_media < 2 || n_media > kMaxMediaWide) return fail(h, "fdtd_set_media: n_media must be in [2, %d], got %d", kMaxMediaWide, n_media);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  std::vector<float2> lut(n_media);
  for (int i = 0; i < n_media; ++i) { lut[i].x = ca[i]; lut[i].y = cb[i]; }
  if (dev_upload(h, &h->lut, (const float2*)lut.data(), lut.size())) return -1;
  h->n_media = n_media;
  h->ca1 = ca[1];
  h->cb1 = cb[1];
  h->cb_host.assign(cb, cb + n_media);
  return 0;
}

extern "C++" {
namespace {
// pack the three index volumes into one word per cell (10 bits per component), derive the
// row-segment words and upload both
template <typename T>
int upload_material(FdtdSolver* h, const T* mat, size_t count) {
  const size_t nc = (size_t)n_cells(h);
  if (count != 3 * nc) return fail(h, "fdtd_set_material: expected %zu entries, got %zu", 3 * nc, count);
  if (h->disp.state == 1) h->tile_cls.clear();
  if (h->n_media == 0) return fail(h, "fdtd_set_material: call fdtd_set_media first");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const GridP& g = h->g;
  const size_t fcount = (size_t)g.sxy * (g.nz + 2);
  std::vector<uint32_t> packed(fcount, kBgWord);                 // ghost planes: background medium
  uint32_t* dst = packed.data() + g.sxy;
  const uint32_t nm = (uint32_t)h->n_media;
  const bool wide = h->n_media > kMaxMedia - 1;           // more media than 10-bit indices name: two words per cell (fdtd_kernels.hpp MatP)
  std::vector<uint32_t> packed_b(wide ? fcount : 0, 1u);
  uint32_t* dst_b = wide ? packed_b.data() + g.sxy : nullptr;
  if (wide) std::fill(packed.begin(), packed.end(), 1u | (1u << 16));
  for (size_t i = 0; i < nc; ++i) {
    const uint32_t m0 = mat[i], m1 = mat[nc + i], m2 = mat[2 * nc + i];
    if (m0 >= nm || m1 >= nm || m2 >= nm) return fail(h, "fdtd_set_material: medium index out of range at cell %zu", i);
    if (wide) { dst[i] = m0 | (m1 << 16); dst_b[i] = m2; }
    else dst[i] = m0 | (m1 << 10) | (m2 << 20);
  }
  h->mat4b = nullptr;
  if (wide) {
    uint32_t* base_b = nullptr;
    if (dev_upload(h, &base_b, (const uint32_t*)packed_b.data(), fcount)) return -1;
    h->mat4b = base_b + g.sxy;
  }
  const int nbx = (g.nx + 255) / 256;
  // (wide layout: a segment's word is the 10-bit packed word of the triple all its cells share — BOTH words of every cell agree — when
  //  its three indices are <= 1023, as those of the background and of ordinary structures are; anything else is kMixedWord.  A packed
  //  word never has its top two bits set.  the WIDE form of fused_step_kernel reads these; the two-pass kernels read none.)
  std::vector<uint32_t> roww((size_t)g.nz * g.ny * nbx);
  for (size_t r = 0; r < (size_t)g.nz * g.ny; ++r)
    for (int bx = 0; bx < nbx; ++bx) {
      const uint32_t* row = dst + r * g.nx;
      const int i0 = bx * 256, i1 = std::min(g.nx, (bx + 1) * 256);
      uint32_t w = row[i0];
      for (int i = i0 + 1; i < i1; ++i) if (row[i] != w) { w = kMixedWord; break; }
      if (wide && w != kMixedWord) {
        const uint32_t* row_b = dst_b + r * g.nx;
        const uint32_t m0 = w & 0xFFFFu, m1 = w >> 16, m2 = row_b[i0];
        for (int i = i0 + 1; i < i1; ++i) if (row_b[i] != m2) { w = kMixedWord; break; }
        if (w != kMixedWord) w = (m0 < (uint32_t)kMaxMedia && m1 < (uint32_t)kMaxMedia && m2 < (uint32_t)kMaxMedia) ? (m0 | (m1 << 10) | (m2 << 20)) : kMixedWord;
      }
      roww[r * nbx + bx] = w;
    }
  uint32_t* base = nullptr;
  if (dev_upload(h, &base, (const uint32_t*)packed.data(), fcount)) return -1;
  if (dev_upload(h, &h->roww, (const uint32_t*)roww.data(), roww.size())) return -1;
  h->roww_host = wide ? std::vector<uint32_t>() : roww;
  h->tile_cls.clear();
  h->mat4 = base + g.sxy;
  return 0;
}
}  // namespace
}  // extern "C++"

int fdtd_set_material(FdtdSolver* h, const uint8_t* mat, size_t bytes) {
  if (!h) return -1;
  return upload_material(h, mat, bytes);
}

int fdtd_set_material16(FdtdSolver* h, const uint16_t* mat, size_t count) {
  if (!h) return -1;
  return upload_material(h, mat, count);
}

int fdtd_set_pml(FdtdSolver* h, int axis, int n_lo, int n_hi, const float* kinv_e, const float* b_e,
                 const float* c_e, const float* kinv_h, const float* b_h, const float* c_h, int n) {
  if (!h) return -1;
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  if (axis < 0 || axis > 2 || n != N[axis]) return fail(h, "fdtd_set_pml: bad axis/length");
  if (n_lo < 0 || n_hi < 0 || n_lo + n_hi > n) return fail(h, "fdtd_set_pml: %d + %d layers exceed %d cells", n_lo, n_hi, n);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  PmlAxisDev& P = h->pml[axis];
  P.n_lo = n_lo; P.n_hi = n_hi; P.n = n;
  // membership of the psi arrays: [0, lo) and [hi0, n); along x rounded outwards to multiples of 4 cells
  // (the tables are identity on the cells this adds), the whole axis when the two ranges would meet
  P.lo = n_lo; P.hi0 = n - n_hi;
  if (axis == 0) { P.lo = (n_lo + 3) / 4 * 4; P.hi0 = (n - n_hi) / 4 * 4; }
  if (P.lo >= P.hi0) { P.lo = n; P.hi0 = n; }
  P.ns = P.lo + (n - P.hi0);
  std::vector<float4> ce(n), chh(n);
  std::vector<float> kve(n), kvh(n);
  for (int i = 0; i < n; ++i) {
    kve[i] = kinv_e[i] - 1.f; kvh[i] = kinv_h[i] - 1.f;
    ce[i].x = kve[i]; ce[i].y = b_e[i]; ce[i].z = c_e[i]; ce[i].w = 0.f;
    chh[i].x = kvh[i]; chh[i].y = b_h[i]; chh[i].z = c_h[i]; chh[i].w = 0.f;
  }
  if (dev_upload(h, &P.ce4, (const float4*)ce.data(), (size_t)n) || dev_upload(h, &P.ch4, (const float4*)chh.data(), (size_t)n) ||
      dev_upload(h, &P.kv_e, (const float*)kve.data(), (size_t)n) || dev_upload(h, &P.b_e, b_e, (size_t)n) ||
      dev_upload(h, &P.c_e, c_e, (size_t)n) || dev_upload(h, &P.kv_h, (const float*)kvh.data(), (size_t)n) ||
      dev_upload(h, &P.b_h, b_h, (size_t)n) || dev_upload(h, &P.c_h, c_h, (size_t)n))
    return -1;
  const size_t other = (size_t)n_cells(h) / (size_t)n;
  P.psi_count = other * P.ns;
  // (x, y axes: one more plane behind the H-side arrays — the ghost slot a z-slab rank receives its lower neighbour's
  //  top-plane psi into, fdtd_kernels.hpp GridP::psi_ghost)
  P.psi_plane = axis < 2 ? P.psi_count / (size_t)h->cfg.nz : 0;
  for (int q = 0; q < 2; ++q)
    for (int s = 0; s < PmlAxisDev::kSets; ++s) {
      if (s >= PmlAxisDev::kH2) P.set(s)[q] = nullptr;            // the lazily allocated sets: on their next use
      else if (P.ns > 0 && dev_alloc(h, &P.set(s)[q], P.set_count(s))) return -1;
    }
  invalidate_pml_blocks(h);
  return 0;
}

int fdtd_set_mirror_plus(FdtdSolver* h, int axis, int wall) {
  if (!h) return -1;
  if (axis < 0 || axis > 2) return fail(h, "fdtd_set_mirror_plus: bad axis %d", axis);
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  if (wall >= 0 && (wall < 2 || wall + 2 > N[axis]))        // (rows padded to a multiple of 4 put more PEC cells behind the ghosts)
    return fail(h, "fdtd_set_mirror_plus: two ghost cells are needed beyond the wall (wall %d of %d cells)", wall, N[axis]);
  if (wall >= 0 && h->cfg.bc[2 * axis + 1] != FDTD_BC_PEC) return fail(h, "fdtd_set_mirror_plus: the plus face of the axis must be declared PEC (plain truncation behind the ghost cells)");
  h->mirror_wall[axis] = wall < 0 ? -1 : wall;
  return 0;
}

int fdtd_set_absorber(FdtdSolver* h, int axis, int n_lo, int n_hi, const float* fb, const float* fc, int n) {
  if (!h) return -1;
  if (axis < 0 || axis > 2) return fail(h, "fdtd_set_absorber: bad axis %d", axis);
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  if (n != N[axis]) return fail(h, "fdtd_set_absorber: axis %d has %d cells, got %d", axis, N[axis], n);
  if (n_lo < 0 || n_hi < 0 || n_lo + n_hi > n) return fail(h, "fdtd_set_absorber: bad layer counts %d + %d", n_lo, n_hi);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  // identity tables on the other axes, so that the kernel always forms the full product
  for (int a = 0; a < 3; ++a) {
    if (h->damp_fb[a]) continue;
    std::vector<float> one((size_t)N[a], 1.0f);
    if (dev_upload(h, &h->damp_fb[a], one.data(), one.size())) return -1;
    if (dev_upload(h, &h->damp_fc[a], one.data(), one.size())) return -1;
    h->damp_lo[a] = 0; h->damp_hi[a] = N[a];
  }
  HIPCHK(h, hipMemcpy(h->damp_fb[axis], fb, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->damp_fc[axis], fc, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  h->damp_lo[axis] = n_lo; h->damp_hi[axis] = n - n_hi;
  h->has_damp = false;
  for (int a = 0; a < 3; ++a) if (h->damp_lo[a] > 0 || h->damp_hi[a] < N[a]) h->has_damp = true;
  return 0;
}

int fdtd_add_ade(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, int n_poles, const float* kap,
                 const float* bet, float cc) {
  if (!h) return -1;
  if (comp < 0 || comp > 2) return fail(h, "fdtd_add_ade: comp must be 0..2");
  if (n_poles < 1 || n_poles > kMaxPoles) return fail(h, "fdtd_add_ade: n_poles must be in [1, %d]", kMaxPoles);
  if (n <= 0) return 0;
  if (h->disp.state == 1) return fail(h, "fdtd_add_ade: the memory terms of this handle's dispersive cells are paged already (a run took step pairs); add every group before the first fdtd_run");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  AdeGroup a{};
  a.comp = comp; a.n = n;
  plane_range(cell_index, n, h->g.sxy, &a.k0, &a.k1);
  {
    bool sorted = true;
    a.strict = true;
    for (int64_t i = 1; i < n && sorted; ++i) { sorted = cell_index[i - 1] <= cell_index[i]; a.strict = a.strict && cell_index[i - 1] != cell_index[i]; }
    a.strict = a.strict && sorted;
    if (sorted) {
      a.plane_off.assign((size_t)h->g.nz + 1, n);
      int64_t i = 0;
      for (int k = 0; k <= h->g.nz; ++k) {
        while (i < n && (long long)cell_index[i] < (long long)k * h->g.sxy) ++i;
        a.plane_off[(size_t)k] = i;
      }
    }
  }
  if (dev_upload(h, &a.cell, cell_index, (size_t)n) || dev_alloc(h, &a.e_old, (size_t)n) ||
      dev_alloc(h, &a.q, (size_t)n * n_poles))
    return -1;
  a.p.n_poles = n_poles; a.p.cc = cc;
  for (int k = 0; k < n_poles; ++k) {
    a.p.kap[k].x = kap[2 * k]; a.p.kap[k].y = kap[2 * k + 1];
    a.p.bet[k].x = bet[2 * k]; a.p.bet[k].y = bet[2 * k + 1];
  }
  h->ade.push_back(a);
  return 0;
}

extern "C++" {
namespace {
// the fdtd_add_* of the whole-grid lists: every listed node, and every neighbour slot that is not kNoNode, is a cell of the grid
int check_list_nodes(FdtdSolver* h, const char* who, const uint32_t* cell, int64_t n, const uint32_t* nbr = nullptr, int slots = 0) {
  const uint64_t ncell = (uint64_t)n_cells(h);
  for (int64_t i = 0; i < n; ++i) if (cell[i] >= ncell) return fail(h, "%s: cell index out of range", who);
  for (int64_t q = 0; q < slots * n; ++q)
    if (nbr[q] != kNoNode && nbr[q] >= ncell) return fail(h, "%s: neighbour index out of range", who);
  return 0;
}
int add_aniso(FdtdSolver* h, const char* who, int comp, int64_t n, const uint32_t* cell_index, const uint32_t* nbr_index,
              const float* w_new, const float* w_old, const uint8_t* wrap) {
  if (!h) return -1;
  if (comp < 0 || comp > 2) return fail(h, "%s: comp must be 0..2", who);
  if (n <= 0) return 0;
  if (check_list_nodes(h, who, cell_index, n, nbr_index, 8)) return -1;
  if (wrap)
    for (int64_t q = 0; q < 8 * n; ++q) {
      const int c = wrap[q];
      if (c >= kWrapCodes || (c & 3) == 3 || ((c >> 2) & 3) == 3 || ((c >> 4) & 3) == 3)
        return fail(h, "%s: bad wrap code %d", who, c);
    }
  HIPCHK(h, hipSetDevice(h->cfg.device));
  AnisoGroup a{};
  a.comp = comp; a.n = n;
  if (dev_upload(h, &a.cell, cell_index, (size_t)n) || dev_upload(h, &a.nbr, nbr_index, (size_t)8 * n) ||
      dev_upload(h, &a.w_new, w_new, (size_t)8 * n) || dev_upload(h, &a.w_old, w_old, (size_t)8 * n) ||
      dev_alloc(h, &a.old, (size_t)8 * n) || dev_alloc(h, &a.delta, (size_t)n) ||
      (wrap && dev_upload(h, &a.wrap, wrap, (size_t)8 * n)))
    return -1;
  h->aniso.push_back(a);
  return 0;
}
}  // namespace
}  // extern "C++"

int fdtd_add_aniso(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, const uint32_t* nbr_index, const float* w_new,
                   const float* w_old) {
  return add_aniso(h, "fdtd_add_aniso", comp, n, cell_index, nbr_index, w_new, w_old, nullptr);
}

int fdtd_add_aniso_bloch(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, const uint32_t* nbr_index,
                         const float* w_new, const float* w_old, const uint8_t* wrap) {
  if (h && !wrap) return fail(h, "fdtd_add_aniso_bloch: no wrap codes");
  return add_aniso(h, "fdtd_add_aniso_bloch", comp, n, cell_index, nbr_index, w_new, w_old, wrap);
}

int fdtd_add_modulation(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, const float* ca, const float* eps_bar,
                        const float* s_bar, const float* d_eps, const float* d_s, double omega_eps, double omega_sigma) {
  if (!h) return -1;
  if (comp < 0 || comp > 2) return fail(h, "fdtd_add_modulation: comp must be 0..2");
  if (n <= 0) return 0;
  if (refuse_lists_on_z_slabs(h, h, "fdtd_add_modulation", true, kModulation)) return -1;
  if (n_lists(h, kNonlinear)) return fail(h, "fdtd_add_modulation: time-modulated media are not available together with nonlinear media");
  if (!std::isfinite(omega_eps) || !std::isfinite(omega_sigma)) return fail(h, "fdtd_add_modulation: omega must be finite");
  if (check_list_nodes(h, "fdtd_add_modulation", cell_index, n)) return -1;
  for (int64_t i = 0; i < n; ++i) {
    // (the kernel divides by eps^{n+1} + s: the largest swing of both must leave it positive)
    const double swing = std::hypot((double)d_eps[2 * i], (double)d_eps[2 * i + 1]) + std::hypot((double)d_s[2 * i], (double)d_s[2 * i + 1]);
    if (!((double)eps_bar[i] + (double)s_bar[i] - swing > 0.0))
      return fail(h, "fdtd_add_modulation: node %lld: eps_bar + s_bar = %g does not exceed the modulation's swing %g", (long long)i,
                  (double)eps_bar[i] + (double)s_bar[i], swing);
  }
  // (a node listed twice in one component would be patched twice; the lists of one component come from disjoint media)
  HIPCHK(h, hipSetDevice(h->cfg.device));
  ModGroup m{};
  m.comp = comp; m.n = n; m.w_eps = omega_eps; m.w_sig = omega_sigma;
  if (dev_upload(h, &m.cell, cell_index, (size_t)n) || dev_upload(h, &m.ca, ca, (size_t)n) ||
      dev_upload(h, &m.eps_bar, eps_bar, (size_t)n) || dev_upload(h, &m.s_bar, s_bar, (size_t)n) ||
      dev_upload(h, &m.d_eps, reinterpret_cast<const float2*>(d_eps), (size_t)n) ||
      dev_upload(h, &m.d_s, reinterpret_cast<const float2*>(d_s), (size_t)n) || dev_alloc(h, &m.old, (size_t)n))
    return -1;
  h->modulation.push_back(m);
  return 0;
}

int fdtd_add_pec_conformal(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, const uint32_t* nbr_index, const float* d) {
  if (!h) return -1;
  if (comp < 3 || comp > 5) return fail(h, "fdtd_add_pec_conformal: comp must be 3..5");
  if (n <= 0) return 0;
  if (refuse_lists_on_z_slabs(h, h, "fdtd_add_pec_conformal", true, kConformal)) return -1;
  for (const ConformalGroup& c : h->conformal)
    if (c.comp == comp) return fail(h, "fdtd_add_pec_conformal: component %d has a list already (a face is listed once)", comp);
  if (check_list_nodes(h, "fdtd_add_pec_conformal", cell_index, n, nbr_index, 4)) return -1;
  for (int64_t q = 0; q < 4 * n; ++q)
    if (!std::isfinite(d[q])) return fail(h, "fdtd_add_pec_conformal: weight %lld is not finite", (long long)q);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  ConformalGroup c{};
  c.comp = comp; c.n = n;
  if (dev_upload(h, &c.cell, cell_index, (size_t)n) || dev_upload(h, &c.nbr, nbr_index, (size_t)(4 * n)) ||
      dev_upload(h, &c.d, d, (size_t)(4 * n)))
    return -1;
  h->conformal.push_back(c);
  return 0;
}

int fdtd_add_nonlinear(FdtdSolver* h, int comp, int64_t n, const uint32_t* cell_index, const uint32_t* nbr_index, const float* ca,
                       const float* eps_bar, const float* s_bar, const float* chi3, int num_iters) {
  if (!h) return -1;
  if (comp < 0 || comp > 2) return fail(h, "fdtd_add_nonlinear: comp must be 0..2");
  if (num_iters < 1 || num_iters > 64) return fail(h, "fdtd_add_nonlinear: num_iters must be 1..64");
  if (n <= 0) return 0;
  if (refuse_lists_on_z_slabs(h, h, "fdtd_add_nonlinear", true, kNonlinear)) return -1;
  if (n_lists(h, kModulation)) return fail(h, "fdtd_add_nonlinear: nonlinear media are not available together with time-modulated media");
  for (const NonlinearGroup& g : h->nonlinear)
    if (g.comp == comp) return fail(h, "fdtd_add_nonlinear: component %d has a list already (a node is listed once)", comp);
  if (n_lists(h, kNonlinear) && h->nonlinear_iters != num_iters)
    return fail(h, "fdtd_add_nonlinear: num_iters = %d, the handle's lists have %d (one value per handle)", num_iters, h->nonlinear_iters);
  if (check_list_nodes(h, "fdtd_add_nonlinear", cell_index, n, nbr_index, 8)) return -1;
  std::vector<float> den0((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(chi3[i])) return fail(h, "fdtd_add_nonlinear: node %lld: chi3 is not finite", (long long)i);
    den0[(size_t)i] = eps_bar[i] + s_bar[i];
    if (!(den0[(size_t)i] > 0.0f)) return fail(h, "fdtd_add_nonlinear: node %lld: eps_bar + s_bar = %g is not positive", (long long)i, (double)den0[(size_t)i]);
    // (the kernel's form of the iterate rests on Ca = (eps_bar - s_bar) / (eps_bar + s_bar): the three must be one table entry's)
    const double ca_of = ((double)eps_bar[i] - (double)s_bar[i]) / ((double)eps_bar[i] + (double)s_bar[i]);
    if (!(std::fabs(ca_of - (double)ca[i]) <= 1e-5))
      return fail(h, "fdtd_add_nonlinear: node %lld: ca = %g is not (eps_bar - s_bar) / (eps_bar + s_bar) = %g", (long long)i, (double)ca[i], ca_of);
  }
  HIPCHK(h, hipSetDevice(h->cfg.device));
  NonlinearGroup g{};
  g.comp = comp; g.n = n;
  if (dev_upload(h, &g.cell, cell_index, (size_t)n) || dev_upload(h, &g.nbr, nbr_index, (size_t)(8 * n)) ||
      dev_upload(h, &g.den0, (const float*)den0.data(), (size_t)n) || dev_upload(h, &g.chi3, chi3, (size_t)n) ||
      dev_alloc(h, &g.old, (size_t)n) || dev_alloc(h, &g.i_old, (size_t)n) || dev_alloc(h, &g.lin, (size_t)n) ||
      dev_alloc(h, &g.next, (size_t)n))
    return -1;
  h->nonlinear.push_back(g);
  h->nonlinear_iters = num_iters;
  return 0;
}

int fdtd_add_point_source(FdtdSolver* h, int64_t n, const int32_t* comp, const uint32_t* cell, const float* w_re,
                          const float* w_im, int64_t n_steps, const float* wave_e, const float* wave_h) {
  if (!h) return -1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const uint64_t ncell = (uint64_t)n_cells(h);
  // Entries that address the same node are merged (their weights multiply the same waveform), so the
  // kernel's plain read-modify-write touches every node once: no race, no atomics, repeatable bits.
  std::map<std::pair<int32_t, uint32_t>, std::pair<double, double>> merged;
  for (int64_t i = 0; i < n; ++i) {
    if (comp[i] < 0 || comp[i] > 5) return fail(h, "fdtd_add_point_source: bad component %d", comp[i]);
    if (cell[i] >= ncell) return fail(h, "fdtd_add_point_source: cell index out of range");
    auto& acc = merged[{comp[i], cell[i]}];
    acc.first += (double)w_re[i];
    acc.second += (double)w_im[i];
  }
  PointSrc s{};
  s.n_steps = n_steps;
  std::vector<float> re[2], im[2];      // [H side?]
  for (const auto& kv : merged) {       // each side keeps the map's order: by component, then by cell
    const int hs = kv.first.first < 3 ? 0 : 1;
    PointSide& P = hs ? s.h : s.e;
    P.host_comp.push_back(kv.first.first); P.host_cell.push_back(kv.first.second);
    re[hs].push_back((float)kv.second.first); im[hs].push_back((float)kv.second.second);
  }
  auto upload = [&](PointSide& P, const std::vector<float>& wre, const std::vector<float>& wim, const float* wave) {
    P.n = (long long)P.host_comp.size();
    plane_range(P.host_cell.data(), P.n, h->g.sxy, &P.k0, &P.k1);
    return P.n && (dev_upload(h, &P.comp, (const int32_t*)P.host_comp.data(), P.host_comp.size()) ||
                   dev_upload(h, &P.cell, (const uint32_t*)P.host_cell.data(), P.host_cell.size()) ||
                   dev_upload(h, &P.wre, (const float*)wre.data(), wre.size()) || dev_upload(h, &P.wim, (const float*)wim.data(), wim.size()) ||
                   dev_upload(h, &P.wave, reinterpret_cast<const float2*>(wave), (size_t)n_steps));
  };
  if (upload(s.e, re[0], im[0], wave_e) || upload(s.h, re[1], im[1], wave_h)) return -1;
  h->psrc.push_back(s);
  return 0;
}

namespace {
// group a TFSF correction list by target node (component, cell), entries of a node in their given order
int build_tfsf_list(FdtdSolver* h, TfsfList& L, int64_t n, const int32_t* comp, const uint32_t* cell, const float* w,
                    const int32_t* aux, int n_aux_max) {
  if (n <= 0) return 0;
  const uint64_t ncell = (uint64_t)n_cells(h);
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (comp[i] < 0 || comp[i] > 5) return fail(h, "fdtd_add_tfsf: bad component %d", comp[i]);
    if (cell[i] >= ncell) return fail(h, "fdtd_add_tfsf: cell index out of range");
    if (aux[i] < 0 || aux[i] > n_aux_max) return fail(h, "fdtd_add_tfsf: auxiliary index out of range");
    order[(size_t)i] = i;
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return comp[x] != comp[y] ? comp[x] < comp[y] : cell[x] < cell[y];
  });
  std::vector<int32_t> tc, st, ax((size_t)n);
  std::vector<uint32_t> tl;
  std::vector<float> ww((size_t)n);
  for (int64_t e = 0; e < n; ++e) {
    const int64_t i = order[(size_t)e];
    if (e == 0 || comp[i] != tc.back() || cell[i] != tl.back()) { tc.push_back(comp[i]); tl.push_back(cell[i]); st.push_back((int32_t)e); }
    ww[(size_t)e] = w[i];
    ax[(size_t)e] = aux[i];
  }
  st.push_back((int32_t)n);
  L.n = (long long)tc.size();
  plane_range(tl.data(), L.n, h->g.sxy, &L.k0, &L.k1);
  if (dev_upload(h, &L.comp, (const int32_t*)tc.data(), tc.size()) || dev_upload(h, &L.cell, (const uint32_t*)tl.data(), tl.size()) ||
      dev_upload(h, &L.start, (const int32_t*)st.data(), st.size()) || dev_upload(h, &L.w, (const float*)ww.data(), ww.size()) ||
      dev_upload(h, &L.aux, (const int32_t*)ax.data(), ax.size()))
    return -1;
  return 0;
}
}  // namespace

int fdtd_add_tfsf(FdtdSolver* h, int n_aux, const float* ae, const float* be, const float* ah, const float* bh,
                  int src_cell, int64_t n_steps, const float* wave, int64_t n_e, const int32_t* e_comp,
                  const uint32_t* e_index, const float* e_w, const int32_t* e_aux, int64_t n_h,
                  const int32_t* h_comp, const uint32_t* h_index, const float* h_w, const int32_t* h_aux) {
  if (!h) return -1;
  if (n_aux < 4 || src_cell < 1 || src_cell >= n_aux) return fail(h, "fdtd_add_tfsf: bad auxiliary grid");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  Tfsf t{};
  t.n_aux = n_aux; t.src_cell = src_cell;
  t.n_steps = n_steps;
  if (dev_upload(h, &t.ae, ae, (size_t)n_aux + 1) || dev_upload(h, &t.be, be, (size_t)n_aux + 1) ||
      dev_upload(h, &t.ah, ah, (size_t)n_aux) || dev_upload(h, &t.bh, bh, (size_t)n_aux) ||
      dev_alloc(h, &t.e1, (size_t)n_aux + 1) || dev_alloc(h, &t.h1, (size_t)n_aux) ||
      dev_alloc(h, &t.e1c, (size_t)n_aux + 1) || dev_alloc(h, &t.h1c, (size_t)n_aux) ||
      dev_upload(h, &t.wave, wave, (size_t)n_steps))
    return -1;
  // E-side corrections read h1 (n_aux entries), H-side ones e1 (n_aux + 1 entries)
  if (build_tfsf_list(h, t.e, n_e, e_comp, e_index, e_w, e_aux, n_aux - 1) ||
      build_tfsf_list(h, t.h, n_h, h_comp, h_index, h_w, h_aux, n_aux))
    return -1;
  h->tfsf.push_back(t);
  return 0;
}

}  // extern "C"
namespace {
// What every fdtd_add_*monitor starts with (`who` = the entry point, for messages): the checks of the handle (`cut` != nullptr:
// the form needs its whole box on one handle, and a z-slab would cut that surface / box), of the components, the index box and
// the steps; then `m`'s comps, box, cells and steps, the extents of the box, and the mark its device memory is counted from.
int monitor_begin(FdtdSolver* h, const char* who, const char* cut, int n_comps, const int32_t* comps, const int32_t lo[3],
                  const int32_t hi[3], int64_t n_rec, const int64_t* steps, Monitor* m, int ext[3]) {
  if (cut && (h->comm || h->cfg.bc[4] == FDTD_BC_NEIGHBOR || h->cfg.bc[5] == FDTD_BC_NEIGHBOR))
    return fail(h, "%s: not available on z-slab handles (the %s would be cut between ranks)", who, cut);
  if (n_comps < 1 || n_comps > 6) return fail(h, "%s: n_comps must be 1..6", who);
  if (!comps || !lo || !hi || n_rec < 0 || (n_rec && !steps)) return fail(h, "%s: bad argument", who);
  for (int c = 0; c < n_comps; ++c) if (comps[c] < 0 || comps[c] > 5) return fail(h, "%s: bad component %d", who, comps[c]);
  const int N[3] = {h->g.nx, h->g.ny, h->g.nz};
  for (int a = 0; a < 3; ++a) {
    if (lo[a] < 0 || hi[a] > N[a] || hi[a] <= lo[a]) return fail(h, "%s: box [%d,%d) outside axis %d of %d cells", who, lo[a], hi[a], a, N[a]);
    ext[a] = hi[a] - lo[a];
  }
  m->comps.assign(comps, comps + n_comps);
  m->box.lo0 = lo[0]; m->box.lo1 = lo[1]; m->box.lo2 = lo[2];
  m->box.nx = ext[0]; m->box.ny = ext[1]; m->box.nz = ext[2];
  m->cells = (long long)ext[0] * ext[1] * ext[2];
  m->steps.assign(steps, steps + n_rec);
  for (size_t i = 1; i < m->steps.size(); ++i)
    if (m->steps[i] <= m->steps[i - 1]) return fail(h, "%s: steps must be strictly increasing", who);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  m->mark = h->stats.device_bytes;
  return 0;
}
// what the handle has allocated since the monitor's mark is `what` (kBytes*) of the monitor
void took(const FdtdSolver* h, Monitor& m, int what) {
  m.held[what] += h->stats.device_bytes - m.mark;
  m.held[kBytesTotal] += h->stats.device_bytes - m.mark;
  m.mark = h->stats.device_bytes;
}
int monitor_end(FdtdSolver* h, const Monitor& m) {
  h->mons.push_back(m);
  return (int)h->mons.size() - 1;
}
// A device-side monitor added between runs skips the steps already done — their part of the result stays zero, a DFT accumulates
// from now on — until fdtd_reset.  (fdtd_add_monitor's do not.)
void skip_done_steps(const FdtdSolver* h, Monitor& m) {
  while (m.next < m.steps.size() && m.steps[m.next] < h->step) ++m.next;
}
// The staging ring of a ring monitor (comps, cells and steps set): as many records as the budget holds, at least two (a step pair
// records two steps), no more than there are.  (Like fdtd_add_monitor: what a failure has allocated stays with the handle until
// fdtd_destroy.)
int ring_setup(FdtdSolver* h, Monitor& m, int64_t staging_bytes) {
  skip_done_steps(h, m);
  m.reduced = m.next;
  const size_t rec_floats = m.comps.size() * (size_t)m.cells, rec_bytes = rec_floats * sizeof(float);
  const size_t budget = staging_bytes > 0 ? (size_t)staging_bytes : ((size_t)32 << 20);
  m.ring = std::max<size_t>(2, std::min<size_t>(std::min<size_t>(budget / rec_bytes, (size_t)kFluxMaxRing), std::max<size_t>(m.steps.size(), 2)));
  m.data_bytes = m.ring * rec_bytes;
  float* stage = nullptr;
  if (dev_alloc(h, &stage, m.ring * rec_floats)) return -1;
  m.data = stage;
  took(h, m, kBytesRecords);
  return 0;
}
// `n` taps along axis `a` of a box of `ext` cells (`of`: whose, for the message): every tap that is read (weight != 0) must lie
// inside the box; no weight may be NaN.
int check_taps(FdtdSolver* h, const char* who, const char* of, int a, size_t n, const int32_t* idx, const float* w, int ext) {
  for (size_t t = 0; t < n; ++t)
    if (!(w[t] == w[t]) || (w[t] != 0.0f && (idx[t] < 0 || idx[t] >= ext)))
      return fail(h, "%s: tap %zu of %saxis %d (index %d, weight %g) outside the box of %d cells", who, t, of, a, idx[t], (double)w[t], ext);
  return 0;
}
// The tap tables of a sparse monitor: component after component and inside a component axis after axis [n_targets][per] taps into
// a box of `ext` cells (per = 2: colocation taps; kLatticeTaps: those of a lattice DFT monitor).  Checks them, fills where each component's tables start, its node counts, where it starts inside a record
// and the total, and uploads them (the monitor's kBytesTables).
int tap_tables(FdtdSolver* h, const char* who, Monitor& m, const int ext[3], const int32_t* n_targets, const int32_t* tap_index,
               const float* tap_weight, TapTables* T, int per = 2) {
  size_t n_taps = 0;
  T->nodes = 0;
  for (size_t c = 0; c < m.comps.size(); ++c) {
    char of[32];
    snprintf(of, sizeof(of), "component %d, ", m.comps[c]);
    long long nodes = 1;
    for (int a = 0; a < 3; ++a) {
      const int nt = n_targets[3 * c + a];
      if (nt < 1 || nt > (1 << 24)) return fail(h, "%s: %d nodes of component %d along axis %d", who, nt, m.comps[c], a);
      T->off[c][a] = (int)n_taps; T->nt[c][a] = nt;
      if (check_taps(h, who, of, a, (size_t)per * nt, tap_index + n_taps, tap_weight + n_taps, ext[a])) return -1;
      n_taps += (size_t)per * nt;
      nodes *= nt;
    }
    T->out_off[c] = T->nodes;
    T->nodes += nodes;
  }
  int* di = nullptr; float* dw = nullptr;
  if (dev_upload(h, &di, (const int*)tap_index, n_taps) || dev_upload(h, &dw, tap_weight, n_taps)) return -1;
  T->idx = di; T->w = dw;
  took(h, m, kBytesTables);
  return 0;
}
}  // namespace
extern "C" {

int fdtd_add_monitor(FdtdSolver* h, int kind, int n_comps, const int32_t* comps, const int32_t lo[3],
                     const int32_t hi[3], int64_t n_rec, const int64_t* steps, int nf, const float* phase_e,
                     const float* phase_h) {
  if (!h) return -1;
  if (kind == FDTD_MON_FLUX_TIME) return fail(h, "fdtd_add_monitor: FDTD_MON_FLUX_TIME monitors are added by fdtd_add_flux_time_monitor");
  if (kind == FDTD_MON_TIME_SPARSE) return fail(h, "fdtd_add_monitor: FDTD_MON_TIME_SPARSE monitors are added by fdtd_add_field_time_monitor");
  if (kind == FDTD_MON_DFT_SPARSE) return fail(h, "fdtd_add_monitor: FDTD_MON_DFT_SPARSE monitors are added by fdtd_add_field_dft_monitor");
  if (kind == FDTD_MON_DFT_LATTICE) return fail(h, "fdtd_add_monitor: FDTD_MON_DFT_LATTICE monitors are added by fdtd_add_lattice_dft_monitor");
  if (kind != FDTD_MON_TIME && kind != FDTD_MON_DFT) return fail(h, "fdtd_add_monitor: bad kind %d", kind);
  Monitor m;
  int ext[3];
  if (monitor_begin(h, "fdtd_add_monitor", nullptr, n_comps, comps, lo, hi, n_rec, steps, &m, ext)) return -1;
  if (kind == FDTD_MON_DFT && nf < 1) return fail(h, "fdtd_add_monitor: a DFT monitor needs frequencies");
  m.kind = kind;
  m.nf = nf;
  if (kind == FDTD_MON_TIME) {
    m.data_bytes = (size_t)n_rec * n_comps * m.cells * sizeof(float);
    float* d = nullptr;
    if (dev_alloc(h, &d, (size_t)n_rec * n_comps * m.cells)) return -1;
    m.data = d;
    took(h, m, kBytesRecords);
  } else {
    m.data_bytes = (size_t)nf * n_comps * m.cells * sizeof(float2);
    float2* d = nullptr;
    if (dev_alloc(h, &d, (size_t)nf * n_comps * m.cells)) return -1;
    m.data = d;
    took(h, m, kBytesRecords);
    if (dev_upload(h, &m.phase_e, reinterpret_cast<const float2*>(phase_e), (size_t)n_rec * nf) ||
        dev_upload(h, &m.phase_h, reinterpret_cast<const float2*>(phase_h), (size_t)n_rec * nf))
      return -1;
    took(h, m, kBytesTables);
  }
  return monitor_end(h, m);
}

int fdtd_add_flux_time_monitor(FdtdSolver* h, int axis, float sign, const int32_t lo[3], const int32_t hi[3], int64_t n_rec,
                               const int64_t* steps, const int32_t n_nodes[3], const int32_t* tap_index, const float* tap_weight,
                               const float* wu, const float* wv, int64_t staging_bytes) {
  if (!h) return -1;
  if (axis < 0 || axis > 2) return fail(h, "fdtd_add_flux_time_monitor: bad axis %d", axis);
  const int t1 = (axis + 1) % 3, t2 = (axis + 2) % 3;
  const int32_t comps[4] = {t1, t2, 3 + t1, 3 + t2};
  Monitor m;
  int ext[3];
  if (monitor_begin(h, "fdtd_add_flux_time_monitor", "surface", 4, comps, lo, hi, n_rec, steps, &m, ext)) return -1;
  if (!n_nodes || !tap_index || !tap_weight || !wu || !wv) return fail(h, "fdtd_add_flux_time_monitor: bad argument");
  const int u = axis == 0 ? 1 : 0;                             // the lower tangential axis (wu), the other one takes wv
  size_t tap_off[3], n_taps = 0;                               // per axis [4][nt][2] taps: eight per node
  for (int a = 0; a < 3; ++a) {
    if (n_nodes[a] < 1 || (a == axis && n_nodes[a] != 1)) return fail(h, "fdtd_add_flux_time_monitor: %d nodes along axis %d", n_nodes[a], a);
    if (check_taps(h, "fdtd_add_flux_time_monitor", "", a, (size_t)8 * n_nodes[a], tap_index + n_taps, tap_weight + n_taps, ext[a])) return -1;
    tap_off[a] = n_taps;
    n_taps += (size_t)8 * n_nodes[a];
  }
  m.kind = FDTD_MON_TIME;
  m.form = MonForm::FluxRing;
  if (ring_setup(h, m, staging_bytes)) return -1;
  float *stage = reinterpret_cast<float*>(m.data), *result = nullptr, *partial = nullptr;
  if (dev_alloc(h, &result, (size_t)n_rec)) return -1;
  m.result_bytes = (size_t)n_rec * sizeof(float);
  took(h, m, kBytesResult);
  FluxMonP& p = m.fp;
  const long long nodes = (long long)n_nodes[0] * n_nodes[1] * n_nodes[2];
  p.tiles = (int)((nodes + kFluxTile - 1) / kFluxTile);
  if (dev_alloc(h, &partial, m.ring * (size_t)p.tiles)) return -1;
  const float one = 1.0f;
  for (int a = 0; a < 3; ++a) {
    int* di = nullptr; float *dw = nullptr, *dwi = nullptr;
    if (dev_upload(h, &di, (const int*)(tap_index + tap_off[a]), (size_t)8 * n_nodes[a]) ||
        dev_upload(h, &dw, tap_weight + tap_off[a], (size_t)8 * n_nodes[a]) ||
        dev_upload(h, &dwi, a == axis ? &one : (a == u ? wu : wv), (size_t)n_nodes[a])) return -1;
    p.idx[a] = di; p.w[a] = dw; p.wi[a] = dwi;
    p.nt[a] = n_nodes[a]; p.b[a] = ext[a];
  }
  p.stage = stage; p.partial = partial; p.result = result;
  p.ring = (int)m.ring;
  p.sign = sign;
  took(h, m, kBytesTables);                                    // (the per-tile partial sums count as tables)
  return monitor_end(h, m);
}

int fdtd_add_field_time_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                                int64_t n_rec, const int64_t* steps, const int32_t* n_targets, const int32_t* tap_index,
                                const float* tap_weight, int64_t staging_bytes) {
  if (!h) return -1;
  const char* who = "fdtd_add_field_time_monitor";
  Monitor m;
  int ext[3];
  if (monitor_begin(h, who, "box", n_comps, comps, lo, hi, n_rec, steps, &m, ext)) return -1;
  if (!n_targets || !tap_index || !tap_weight) return fail(h, "%s: bad argument", who);
  m.kind = FDTD_MON_TIME;
  m.form = MonForm::SparseRing;
  FieldTimeP& p = m.gp;
  if (tap_tables(h, who, m, ext, n_targets, tap_index, tap_weight, &p.t) || ring_setup(h, m, staging_bytes)) return -1;
  if (dev_alloc(h, &p.out, (size_t)n_rec * (size_t)p.t.nodes)) return -1;
  m.result_bytes = (size_t)n_rec * (size_t)p.t.nodes * sizeof(float);
  took(h, m, kBytesResult);
  p.stage = reinterpret_cast<const float*>(m.data);
  for (int a = 0; a < 3; ++a) p.b[a] = ext[a];
  p.n_comps = n_comps; p.ring = (int)m.ring;
  return monitor_end(h, m);
}

}  // extern "C"
namespace {
// fdtd_add_field_dft_monitor and fdtd_add_lattice_dft_monitor: accumulators on the kept nodes alone, `per` taps per node and axis
int add_sparse_dft(FdtdSolver* h, const char* who, MonForm form, int per, int n_comps, const int32_t* comps, const int32_t lo[3],
                   const int32_t hi[3], int64_t n_rec, const int64_t* steps, const int32_t* n_targets, const int32_t* tap_index,
                   const float* tap_weight, int nf, const float* phase_e, const float* phase_h) {
  Monitor m;
  int ext[3];
  if (monitor_begin(h, who, "box", n_comps, comps, lo, hi, n_rec, steps, &m, ext)) return -1;
  if (!n_targets || !tap_index || !tap_weight || (n_rec && (!phase_e || !phase_h))) return fail(h, "%s: bad argument", who);
  if (nf < 1) return fail(h, "%s: a DFT monitor needs frequencies", who);
  m.kind = FDTD_MON_DFT;
  m.form = form;
  m.nf = nf;
  skip_done_steps(h, m);
  // (like fdtd_add_monitor: what a failure below has allocated stays with the handle until fdtd_destroy)
  FieldDftP& p = m.dp;
  if (tap_tables(h, who, m, ext, n_targets, tap_index, tap_weight, &p.t, per)) return -1;
  m.data_bytes = (size_t)nf * (size_t)p.t.nodes * sizeof(float2);
  if (dev_alloc(h, &p.acc, (size_t)nf * (size_t)p.t.nodes)) return -1;
  m.data = p.acc;
  took(h, m, kBytesResult);                                    // (no records: the accumulators are the result)
  if (dev_upload(h, &m.phase_e, reinterpret_cast<const float2*>(phase_e), (size_t)n_rec * nf) ||
      dev_upload(h, &m.phase_h, reinterpret_cast<const float2*>(phase_h), (size_t)n_rec * nf))
    return -1;
  took(h, m, kBytesTables);
  p.nf = nf;
  return monitor_end(h, m);
}
}  // namespace
extern "C" {

int fdtd_add_field_dft_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                               int64_t n_rec, const int64_t* steps, const int32_t* n_targets, const int32_t* tap_index,
                               const float* tap_weight, int nf, const float* phase_e, const float* phase_h) {
  if (!h) return -1;
  return add_sparse_dft(h, "fdtd_add_field_dft_monitor", MonForm::SparseDft, 2, n_comps, comps, lo, hi, n_rec, steps, n_targets, tap_index,
                        tap_weight, nf, phase_e, phase_h);
}

int fdtd_add_lattice_dft_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                                 int64_t n_rec, const int64_t* steps, const int32_t* n_targets, int n_taps, const int32_t* tap_index,
                                 const float* tap_weight, int nf, const float* phase_e, const float* phase_h) {
  if (!h) return -1;
  if (n_taps != kLatticeTaps) return fail(h, "fdtd_add_lattice_dft_monitor: n_taps must be %d, got %d", kLatticeTaps, n_taps);
  return add_sparse_dft(h, "fdtd_add_lattice_dft_monitor", MonForm::LatticeDft, kLatticeTaps, n_comps, comps, lo, hi, n_rec, steps, n_targets,
                        tap_index, tap_weight, nf, phase_e, phase_h);
}

}  // extern "C"
namespace {
// fdtd_set_lattice_flux_weights and fdtd_lattice_flux: the monitor `id` as a lattice DFT monitor on a handle that may reduce it
Monitor* lattice_flux_monitor(FdtdSolver* h, const char* who, int id) {
  if (h->comm || h->cfg.bc[4] == FDTD_BC_NEIGHBOR || h->cfg.bc[5] == FDTD_BC_NEIGHBOR) {
    fail(h, "%s: not available on z-slab handles (the surface would be cut between ranks)", who);
    return nullptr;
  }
  if (h->bloch_pair) { fail(h, "%s: not available on the handles of a Bloch pair (complex fields)", who); return nullptr; }
  if (id < 0 || id >= (int)h->mons.size()) { fail(h, "%s: bad id %d", who, id); return nullptr; }
  if (h->mons[id].form != MonForm::LatticeDft) {
    fail(h, "%s: monitor %d has no lattice accumulators (it was not added by fdtd_add_lattice_dft_monitor)", who, id);
    return nullptr;
  }
  return &h->mons[id];
}
}  // namespace
extern "C" {

int fdtd_set_lattice_flux_weights(FdtdSolver* h, int id, int axis, double sign, const int32_t n[3], const double* w0, const double* w1,
                                  const double* w2) {
  if (!h) return -1;
  const char* who = "fdtd_set_lattice_flux_weights";
  Monitor* m = lattice_flux_monitor(h, who, id);
  if (!m) return -1;
  if (axis < 0 || axis > 2 || !n || !w0 || !w1 || !w2) return fail(h, "%s: bad argument", who);
  if (m->has_flux) return fail(h, "%s: monitor %d has its weights already", who, id);
  // the four tangential components of the surface, in whatever order the monitor holds them; every one on the same lattice
  const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
  const int want[4] = {a1, a2, 3 + a1, 3 + a2};
  const TapTables& T = m->dp.t;
  LatticeFluxP p{};
  if (m->comps.size() != 4) return fail(h, "%s: monitor %d holds %zu components, a surface holds its four tangential ones", who, id, m->comps.size());
  for (int q = 0; q < 4; ++q) {
    int slot = -1;
    for (int c = 0; c < 4; ++c) if (m->comps[c] == want[q]) slot = c;
    if (slot < 0) return fail(h, "%s: monitor %d does not hold component %d, tangential to a surface normal to axis %d", who, id, want[q], axis);
    for (int a = 0; a < 3; ++a)
      if (T.nt[slot][a] != n[a] || (a == axis && n[a] != 1))
        return fail(h, "%s: %d weights along axis %d, component %d of monitor %d keeps %d nodes there", who, n[a], a, want[q], id, T.nt[slot][a]);
    p.off[q] = T.out_off[slot];
  }
  const double* w[3] = {w0, w1, w2};
  for (int a = 0; a < 3; ++a)
    for (int i = 0; i < n[a]; ++i)
      if (!(w[a][i] == w[a][i])) return fail(h, "%s: weight %d along axis %d is not a number", who, i, a);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  m->mark = h->stats.device_bytes;
  for (int a = 0; a < 3; ++a) {
    double* dw = nullptr;
    if (dev_upload(h, &dw, w[a], (size_t)n[a])) return -1;
    p.w[a] = dw; p.n[a] = n[a];
  }
  if (dev_alloc(h, &p.out, (size_t)m->nf)) return -1;
  took(h, *m, kBytesTables);
  p.acc = m->dp.acc; p.nodes = T.nodes;
  p.half_sign = 0.5 * sign;
  m->lp = p;
  m->has_flux = true;
  return 0;
}

int fdtd_lattice_flux(FdtdSolver* h, int id, double* out) {
  if (!h) return -1;
  const char* who = "fdtd_lattice_flux";
  Monitor* m = lattice_flux_monitor(h, who, id);
  if (!m) return -1;
  if (!out) return fail(h, "%s: bad argument", who);
  if (!m->has_flux) return fail(h, "%s: monitor %d has no integration weights (fdtd_set_lattice_flux_weights)", who, id);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(lattice_flux_kernel, dim3((unsigned)m->nf), dim3(kLatticeFluxThreads), 0, h->stream, m->lp);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, m->lp.out, (size_t)m->nf * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int fdtd_get_monitor_bytes(FdtdSolver* h, int id, int64_t out[4]) {
  if (!h) return -1;
  if (id < 0 || id >= (int)h->mons.size() || !out) return fail(h, "fdtd_get_monitor_bytes: bad id %d", id);
  std::copy(h->mons[id].held, h->mons[id].held + 4, out);
  return 0;
}

int fdtd_get_monitor(FdtdSolver* h, int id, void* host, size_t bytes) {
  if (!h) return -1;
  if (id < 0 || id >= (int)h->mons.size()) return fail(h, "fdtd_get_monitor: bad id %d", id);
  Monitor& m = h->mons[id];
  if (has_ring(m)) {                   // the reduced series / the gathered nodes
    if (bytes != m.result_bytes) return fail(h, "fdtd_get_monitor: expected %zu bytes, got %zu", m.result_bytes, bytes);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    ring_drain(h, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bytes) HIPCHK(h, hipMemcpy(host, m.result(), bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  if (bytes != m.data_bytes) return fail(h, "fdtd_get_monitor: expected %zu bytes, got %zu", m.data_bytes, bytes);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(host, m.data, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int fdtd_set_field(FdtdSolver* h, int comp, const float* host, size_t bytes) {
  if (!h) return -1;
  if (comp < 0 || comp > 5) return fail(h, "fdtd_set_field: bad component");
  if (bytes != (size_t)n_cells(h) * 4) return fail(h, "fdtd_set_field: expected %zu bytes", (size_t)n_cells(h) * 4);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (h->seam_pending) { flush_seams(h, h->stream); HIPCHK(h, hipStreamSynchronize(h->stream)); }      // (only behind a run that ended in an error)
  HIPCHK(h, hipMemcpy(field_ptr(h, comp), host, bytes, hipMemcpyHostToDevice));
  // the ADE recursion forms Q^{n+1} from E^{n+1} + E^n: E^n of its cells is the value just uploaded
  for (AdeGroup& a : h->ade)
    if (a.comp == comp) {
      hipLaunchKernelGGL(ade_gather_kernel, dim3(nblk(a.n)), dim3(256), 0, h->stream, (const float*)field_ptr(h, comp),
                         (const uint32_t*)a.cell, a.e_old, a.n);
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  // keep single-slab ghost planes consistent with the new interior
  if (h->comm == nullptr) { fill_ghost_h(h, h->stream); fill_ghost_e(h, h->stream); fill_ghost_fused(h, h->stream); HIPCHK(h, hipStreamSynchronize(h->stream)); }
  else if (comp == 0 || comp == 1 || comp == 3 || comp == 4) {
    // with a communicator the ghost planes come from the neighbour: do one exchange now
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (exchange(h, comp < 3, h->comm_stream)) return -1;
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  }
  return 0;
}

int fdtd_get_field(FdtdSolver* h, int comp, float* host, size_t bytes) {
  if (!h) return -1;
  if (comp < 0 || comp > 5) return fail(h, "fdtd_get_field: bad component");
  if (bytes != (size_t)n_cells(h) * 4) return fail(h, "fdtd_get_field: expected %zu bytes", (size_t)n_cells(h) * 4);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  flush_seams(h, h->stream);                 // (only behind a run that ended in an error: fdtd_run returns with nothing pending)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(host, field_ptr(h, comp), bytes, hipMemcpyDeviceToHost));
  return 0;
}

int fdtd_set_shutoff(FdtdSolver* h, int every, double shutoff, int64_t ref_step) {
  if (!h) return -1;
  h->decay_every = every; h->shutoff = shutoff; h->decay_ref = ref_step;
  return 0;
}

int fdtd_comm_unique_id(char id[128]) {
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return fail(nullptr, "ncclGetUniqueId failed");
  std::memcpy(id, &u, 128);
  return 0;
}

int fdtd_comm_init(FdtdSolver* h, const char id[128], int rank, int n_ranks) {
  if (!h) return -1;
  if (rank < 0 || rank >= n_ranks) return fail(h, "fdtd_comm_init: bad rank %d of %d", rank, n_ranks);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  ncclUniqueId u;
  std::memcpy(&u, id, 128);
  if (refuse_whole_grid_monitors(h, h, "fdtd_comm_init")) return -1;
  if (refuse_lists_on_z_slabs(h, h, "fdtd_comm_init", true)) return -1;
  NCCLCHK(h, ncclCommInitRank(&h->comm, n_ranks, u, rank));
  h->rank = rank; h->n_ranks = n_ranks;
  // what the communicator itself reports goes into FdtdStats (bench.py --gpus N prints it: proof that RCCL saw N ranks)
  int cnt = 0, ur = -1;
  NCCLCHK(h, ncclCommCount(h->comm, &cnt));
  NCCLCHK(h, ncclCommUserRank(h->comm, &ur));
  h->stats.comm_ranks = cnt; h->stats.comm_rank = ur;
  return 0;
}

}  // extern "C"
namespace {
// ---- the state that evolves from step to step: ONE table (include/fdtd_hip.h, above fdtd_get_state) ---------------------------------
// fdtd_reset zeroes every section; fdtd_state_bytes, fdtd_get_state and fdtd_set_state walk the Saved ones in this order.
//   Saved:   what the blob of fdtd_get_state holds.  The field and psi pointers a handle calls current ARE the live ones (swap_sets,
//            swap_psi_h, swap_psi_e exchange the pointers), so the section is the live array whatever the step's parity.
//   Scratch: the write sides of the ping-pongs (lazily allocated: a fresh handle may lack them) — every value read from them was
//            written in the same step or pair.  fdtd_set_state zeroes them.
//   Derived: disp.cs = cc S(Q) of every dispersive cell, a function of q alone (ade_kernel, ade2_kernel and disp_qoff_kernel form it
//            with the same operations in the same order).  fdtd_set_state rebuilds it where the handle has paged (state_rebuild_paged).
enum StateRole { kStateSaved, kStateScratch, kStateDerived };
struct StateSection { void* p; size_t bytes; StateRole role; };
std::vector<StateSection> state_sections(FdtdSolver* h) {
  std::vector<StateSection> v;
  for (int c = 0; c < 6; ++c) v.push_back({h->fbase[c], h->field_bytes, kStateSaved});
  for (int c = 0; c < 6; ++c) if (h->fbase2[c]) v.push_back({h->fbase2[c], h->field_bytes, kStateScratch});
  for (int c = 0; c < 6; ++c) if (h->fbase3[c]) v.push_back({h->fbase3[c], h->field_bytes, kStateScratch});
  for (int a = 0; a < 3; ++a) {
    PmlAxisDev& P = h->pml[a];
    if (P.n == 0) continue;
    for (int q = 0; q < 2; ++q)
      for (int s = 0; s < PmlAxisDev::kSets; ++s)
        if (P.set(s)[q]) v.push_back({P.set(s)[q], P.set_count(s) * 4, s == PmlAxisDev::kE || s == PmlAxisDev::kH ? kStateSaved : kStateScratch});
  }
  for (AdeGroup& a : h->ade) {
    v.push_back({a.e_old, (size_t)a.n * 4, kStateSaved});
    v.push_back({a.q, (size_t)a.n * a.p.n_poles * 8, kStateSaved});
  }
  if (h->disp.state == 1) v.push_back({h->disp.cs, (size_t)h->disp.seg.n_blocks * 3 * 256 * sizeof(float), kStateDerived});
  for (Tfsf& t : h->tfsf) {
    v.push_back({t.e1, ((size_t)t.n_aux + 1) * 4, kStateSaved});
    v.push_back({t.h1, (size_t)t.n_aux * 4, kStateSaved});
  }
  for (Monitor& m : h->mons) {
    v.push_back({m.data, m.data_bytes, kStateSaved});
    if (has_ring(m)) v.push_back({m.result(), std::max<size_t>(m.result_bytes, sizeof(float)), kStateSaved});
  }
  return v;
}
std::vector<StateSection> saved_sections(FdtdSolver* h) {
  std::vector<StateSection> v;
  for (const StateSection& s : state_sections(h)) if (s.role == kStateSaved) v.push_back(s);
  return v;
}
size_t state_table_bytes(size_t n_sections, size_t n_monitors) { return sizeof(FdtdStateHeader) + 8 * n_sections + 16 * n_monitors; }
// 64-bit FNV-1a over the words that fix the layout and the meaning of the Saved sections
uint64_t state_fingerprint(const FdtdSolver* h) {
  uint64_t x = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { for (int b = 0; b < 8; ++b) { x ^= (v >> (8 * b)) & 0xff; x *= 1099511628211ull; } };
  mix((uint64_t)h->g.nx); mix((uint64_t)h->g.ny); mix((uint64_t)h->g.nz); mix(h->field_bytes);
  for (int a = 0; a < 3; ++a) {
    const PmlAxisDev& P = h->pml[a];
    mix((uint64_t)P.n_lo); mix((uint64_t)P.n_hi);
    mix(P.ns > 0 ? P.set_count(PmlAxisDev::kE) : 0); mix(P.ns > 0 ? P.set_count(PmlAxisDev::kH) : 0);
  }
  mix(h->ade.size());
  for (const AdeGroup& a : h->ade) { mix((uint64_t)a.comp); mix((uint64_t)a.n); mix((uint64_t)a.p.n_poles); }
  mix(h->tfsf.size());
  for (const Tfsf& t : h->tfsf) mix((uint64_t)t.n_aux);
  mix(h->mons.size());
  for (const Monitor& m : h->mons) { mix((uint64_t)m.kind); mix((uint64_t)m.form); mix(m.data_bytes); mix(m.result_bytes); }
  for (int kind = 0; kind < kListKinds; ++kind) mix(n_lists(h, kind));
  return x;
}
int refuse_state_on_z_slabs(FdtdSolver* h, const char* who) {
  return h->comm ? fail(h, "%s: state save / restore is not available on z-slab handles", who) : 0;
}
// the paged memory terms of a handle that has paged, from the pole states as they stand: the set-up kernel again (it writes the slots
// and the bounding box it found the first time).
// What this RELIES on: disp_qoff_kernel gives cc * S(Q) the bits ade_kernel / ade2_kernel leave in `cs`.  The three write the same
// expression — S += 2 ((kap.x - 1) q.x - kap.y q.y) over the poles in ascending order from 0.f, then cc * S — but two of them in a loop
// unrolled over kMaxPoles and one in a run-time loop, so equal bits need each operation rounded on its own in all three: no FMA
// contraction.  The library is built with -ffp-contract=off (tidy3d_amd/build.py, tests/hipemu/build_emu.py: the flag every bit
// comparison between its schedules rests on); a build without it would break this, and the lazy paging of a restored handle
// (disp_setup) with it.  Held by scenario (d) and the live-handle tests of tests/test_emu_checkpoint.py / test_gpu_checkpoint.py
// (one-, two- and three-pole media).
int state_rebuild_paged(FdtdSolver* h) {
  Disp& D = h->disp;
  if (D.state != 1) return 0;
  const GridP& g = h->g;
  const int nbx = (g.nx + 255) / 256;
  int* box = nullptr;
  if (box_seed_upload(h, &box)) return -1;
  for (AdeGroup& a : h->ade)
    hipLaunchKernelGGL(disp_qoff_kernel, dim3(nblk(a.n)), dim3(256), 0, h->stream, (const uint32_t*)a.cell, a.n, g.nx, g.ny, nbx,
                       (const int*)D.seg.dev, a.comp, (const float2*)a.q, a.p, a.qoff, D.cs, box);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  release_buf(h, box);
  return 0;
}
int state_sync(FdtdSolver* h) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->comm_stream && !h->streams_shared) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  if (h->box_stream) HIPCHK(h, hipStreamSynchronize(h->box_stream));
  return 0;
}
}  // namespace
extern "C" {

int fdtd_reset(FdtdSolver* h) {
  if (!h) return -1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->seam_pending = false;
  h->sweep_words.clear();
  for (const StateSection& s : state_sections(h)) HIPCHK(h, hipMemset(s.p, 0, s.bytes));
  for (Monitor& m : h->mons) { m.next = 0; m.reduced = 0; }
  h->step = 0; h->energy_max = 0.0;
  h->stats.steps_done = 0; h->stats.diverged = 0; h->stats.stopped_early = 0; h->stats.field_decay = 0.0;      // (what a fresh handle reports until its first decay check)
  return 0;
}

int fdtd_state_fingerprint(FdtdSolver* h, uint64_t* out) {
  if (!h) return -1;
  if (!out) return fail(h, "fdtd_state_fingerprint: null argument");
  if (refuse_state_on_z_slabs(h, "fdtd_state_fingerprint")) return -1;
  *out = state_fingerprint(h);
  return 0;
}

int64_t fdtd_state_bytes(FdtdSolver* h) {
  if (!h) return -1;
  if (refuse_state_on_z_slabs(h, "fdtd_state_bytes")) return -1;
  const std::vector<StateSection> sec = saved_sections(h);
  size_t total = state_table_bytes(sec.size(), h->mons.size());
  for (const StateSection& s : sec) total += s.bytes;
  return (int64_t)total;
}

int fdtd_get_state(FdtdSolver* h, void* host, size_t bytes) {
  if (!h) return -1;
  if (refuse_state_on_z_slabs(h, "fdtd_get_state")) return -1;
  const int64_t need = fdtd_state_bytes(h);
  if (!host || bytes < (size_t)need) return fail(h, "fdtd_get_state: buffer of %zu bytes is too small (the state holds %lld)", bytes, (long long)need);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (state_sync(h)) return -1;
  flush_seams(h, h->stream);          // (what fdtd_run does on its way out: nothing pending, no record waiting in a ring)
  ring_drain(h, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const std::vector<StateSection> sec = saved_sections(h);
  FdtdStateHeader hd{};
  std::memcpy(hd.magic, FDTD_STATE_MAGIC, 8);
  hd.version = FDTD_STATE_VERSION;
  hd.fingerprint = state_fingerprint(h);
  hd.step = h->step;
  hd.n_sections = sec.size();
  hd.n_monitors = h->mons.size();
  hd.energy_max = h->energy_max;
  hd.steps_done = h->stats.steps_done; hd.diverged = h->stats.diverged; hd.stopped_early = h->stats.stopped_early;
  hd.field_decay = h->stats.field_decay;
  hd.total_bytes = (uint64_t)need;
  char* out = static_cast<char*>(host);
  std::memcpy(out, &hd, sizeof(hd));
  out += sizeof(hd);
  for (const StateSection& s : sec) { const uint64_t b = s.bytes; std::memcpy(out, &b, 8); out += 8; }
  for (const Monitor& m : h->mons) { const uint64_t v[2] = {m.next, m.reduced}; std::memcpy(out, v, 16); out += 16; }
  for (const StateSection& s : sec) {
    if (s.bytes) HIPCHK(h, hipMemcpy(out, s.p, s.bytes, hipMemcpyDeviceToHost));
    out += s.bytes;
  }
  return 0;
}

int fdtd_set_state(FdtdSolver* h, const void* host, size_t bytes) {
  if (!h) return -1;
  if (refuse_state_on_z_slabs(h, "fdtd_set_state")) return -1;
  // every check in front of the first change
  FdtdStateHeader hd;
  if (!host || bytes < sizeof(hd)) return fail(h, "fdtd_set_state: buffer of %zu bytes is too small for the header (%zu)", bytes, sizeof(hd));
  std::memcpy(&hd, host, sizeof(hd));
  if (std::memcmp(hd.magic, FDTD_STATE_MAGIC, 8) != 0) return fail(h, "fdtd_set_state: bad magic (not a state blob of this library)");
  if (hd.version != FDTD_STATE_VERSION)
    return fail(h, "fdtd_set_state: format version %llu, this library reads %d", (unsigned long long)hd.version, FDTD_STATE_VERSION);
  const uint64_t fp = state_fingerprint(h);
  if (hd.fingerprint != fp)
    return fail(h, "fdtd_set_state: fingerprint %016llx is not this handle's (%016llx): the blob was written by a handle set up differently",
                (unsigned long long)hd.fingerprint, (unsigned long long)fp);
  const std::vector<StateSection> sec = saved_sections(h);
  if (hd.n_sections != sec.size() || hd.n_monitors != h->mons.size())
    return fail(h, "fdtd_set_state: section count %llu / monitor count %llu differ from this handle's %zu / %zu",
                (unsigned long long)hd.n_sections, (unsigned long long)hd.n_monitors, sec.size(), h->mons.size());
  const size_t table = state_table_bytes(sec.size(), h->mons.size());
  if (bytes < table) return fail(h, "fdtd_set_state: buffer of %zu bytes is too small for the section table (%zu)", bytes, table);
  const char* in = static_cast<const char*>(host) + sizeof(hd);
  size_t total = table;
  for (size_t i = 0; i < sec.size(); ++i) {
    uint64_t b;
    std::memcpy(&b, in + 8 * i, 8);
    if (b != sec[i].bytes)
      return fail(h, "fdtd_set_state: section %zu holds %llu bytes, this handle's %zu", i, (unsigned long long)b, sec[i].bytes);
    total += sec[i].bytes;
  }
  if (bytes < total || hd.total_bytes != total)
    return fail(h, "fdtd_set_state: buffer of %zu bytes is too small (the state holds %zu; its header says %llu)", bytes, total,
                (unsigned long long)hd.total_bytes);
  const char* mon_in = in + 8 * sec.size();
  for (size_t i = 0; i < h->mons.size(); ++i) {
    uint64_t v[2];
    std::memcpy(v, mon_in + 16 * i, 16);
    if (v[0] > h->mons[i].steps.size() || v[1] > v[0])
      return fail(h, "fdtd_set_state: monitor %zu at record %llu (reduced %llu) of %zu", i, (unsigned long long)v[0], (unsigned long long)v[1],
                  h->mons[i].steps.size());
  }
  if (hd.step < 0) return fail(h, "fdtd_set_state: step %lld", (long long)hd.step);
  // from here on the handle changes
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (state_sync(h)) return -1;
  h->seam_pending = false;            // (the seam columns arrive with the fields)
  const char* data = static_cast<const char*>(host) + table;
  for (const StateSection& s : sec) {
    if (s.bytes) HIPCHK(h, hipMemcpy(s.p, data, s.bytes, hipMemcpyHostToDevice));
    data += s.bytes;
  }
  for (const StateSection& s : state_sections(h))
    if (s.role == kStateScratch) HIPCHK(h, hipMemset(s.p, 0, s.bytes));
  HIPCHK(h, hipStreamSynchronize(nullptr));
  if (state_rebuild_paged(h)) return -1;
  for (size_t i = 0; i < h->mons.size(); ++i) {
    uint64_t v[2];
    std::memcpy(v, mon_in + 16 * i, 16);
    h->mons[i].next = (size_t)v[0]; h->mons[i].reduced = (size_t)v[1];
  }
  h->step = hd.step; h->energy_max = hd.energy_max;
  h->stats.steps_done = hd.steps_done; h->stats.diverged = (int32_t)hd.diverged; h->stats.stopped_early = (int32_t)hd.stopped_early;
  h->stats.field_decay = hd.field_decay;
  return 0;
}

// ---- fdtd_run ---------------------------------------------------------------------------------------------------------------
// (struct Run, one object per call: fdtd_run.hpp; struct BlochRun, the same for fdtd_run_bloch: fdtd_run_bloch.hpp)
}  // extern "C"
namespace {
#include "fdtd_run.hpp"
#include "fdtd_run_bloch.hpp"
}  // namespace
extern "C" {

int fdtd_run(FdtdSolver* h, int64_t n_steps, FdtdProgressFn progress, void* user) {
  if (!h) return -1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (h->comm && refuse_whole_grid_monitors(h, h, "fdtd_run")) return -1;
  Run r{h, n_steps, progress, user};
  if (r.setup() || r.setup_schedules() || r.setup_pairs()) return -1;
  if (r.loop()) { flush_seams(h, h->stream); return -1; }      // (an error leaves no stale seam columns either)
  return r.finish();
}
// Complex (Bloch-periodic) fields as a (Re, Im) pair of solvers stepped together (struct BlochRun, one object per call: fdtd_run_bloch.hpp)
int fdtd_run_bloch(FdtdSolver* hr, FdtdSolver* hi, int64_t n_steps, const double phase[3], const int n_real[3],
                   FdtdProgressFn progress, void* user) {
  if (!hr || !hi) return -1;
  BlochRun r{hr, hi, n_steps, phase, n_real, progress, user};
  if (r.setup() || r.loop()) return -1;
  return r.finish();
}

int fdtd_set_option(FdtdSolver* h, int key, int value) {
  if (!h) return -1;
  switch (key) {
    case FDTD_OPT_FLAGS: h->cfg.flags = value; return 0;
    case FDTD_OPT_VARIANT: h->cfg.variant = value; return 0;
    case FDTD_OPT_ZCHUNK: if (value < 1) break; h->zchunk = value; h->zchunk_f = value; h->user_geometry = true; return 0;
    case FDTD_OPT_ROWS: if (value < 1 || value > 15) break; h->rows = value > 8 ? 8 : value; h->rows_f = value; h->user_geometry = true; return 0;
    case FDTD_OPT_XCD_REMAP: if (value > 1024) break; h->xcd_remap = value < 0 ? -1 : value; return 0;
    case FDTD_OPT_PML_FUSED: h->pml_fused = value < 0 ? -1 : (value & 7); invalidate_pml_blocks(h); return 0;
    case FDTD_OPT_BND_PLANES: h->bnd_planes = value > 0 ? value : 0; return 0;
    case FDTD_OPT_AUTOTUNE: h->autotune = value < 0 ? 0 : (value > 2 ? 1 : value); if (value) h->tuned = false; return 0;
    case FDTD_OPT_MEM_HINTS: h->mem_hints = value != 0; return 0;
    case FDTD_OPT_PLACEMENT_TRIES: if (value < 0 || (value % 100) > 8) break; h->placement_tries = value; h->placement_done = false; return 0;
    case FDTD_OPT_LDS_PAD: if (value < 0 || value > 120000) break; h->lds_pad = value; return 0;
    case FDTD_OPT_TBLOCK: h->tblock = value < 0 ? -1 : value; return 0;
    case FDTD_OPT_EDGE_ZCHUNK: h->edge_zchunk = value < 0 ? -1 : value; return 0;
    case FDTD_OPT_GRAPH: h->use_graph = value < 0 ? -1 : (value != 0); return 0;
    case FDTD_OPT_TWOSTEP: {
      if (value <= 0) { h->twostep_w = value < 0 ? -1 : 0; h->twostep_zc = 0; return 0; }
      const int w = value % 64, zc = (value / 64) % 1024;
      if (w < 4 || w > 16) return fail(h, "FDTD_OPT_TWOSTEP: %d waves per workgroup (4 ... 16)", w);
      h->twostep_w = w;
      h->twostep_zc = zc;
      return 0;
    }
    case FDTD_OPT_PML_SPLIT: h->pml_split = value < 0 ? -1 : (value != 0); return 0;
    case FDTD_OPT_SHELL_PAIRS: h->shell_on = value < 0 ? -1 : value; return 0;
    case FDTD_OPT_STRIP: if (value % 64 < 1 || (value / 64 != 3 && value / 64 != 4)) break; h->strip_zc = value % 64; h->strip_occ = value / 64; return 0;
    case FDTD_OPT_SHELL2: h->shell2_on = value < 0 ? -1 : (value > 3 ? 1 : value); return 0;
    case FDTD_OPT_DEBUG_SYNC: h->debug_sync = value != 0; return 0;
    case FDTD_OPT_TILE_SPLIT: h->tile_split = value < 0 ? -1 : (value != 0); return 0;
    case FDTD_OPT_SRC_PAGED:
      h->spg_on = value < 0 ? -1 : (value != 0);
      if (h->spg.state == -1 && value != 0) h->spg.state = 0;
      return 0;
    case FDTD_OPT_SLAB_BOXES_FIRST: if (value < 0 || value > 3) break; h->slab_boxes_first = value; return 0;
    case FDTD_OPT_WHATIF: if (value < 0 || value > 19) break; h->whatif = value; return 0;
    case FDTD_OPT_SEAM_DEFER: if (value > 2) break; h->seam_defer = value < 0 ? -1 : value; return 0;
    case FDTD_OPT_AXIS_SHIFT: if (value < 0 || value > 2) break; h->axis_shift = value; return 0;
    case FDTD_OPT_DISP:
      if (h->disp.state == 1 && value == 0) break;       // (every ADE launch keeps the paged memory terms by now: set it before the first run)
      h->disp_on = value < 0 ? -1 : (value != 0);
      if (h->disp.state == -1 && value != 0) h->disp.state = 0;
      return 0;
    case FDTD_OPT_SHELL2_SHAPE: {
      // lanes per row of the wide boxes (3 ... 64) + 128 * their waves per workgroup (1 ... 8) + 1024 * their planes per chunk (0 = by box)
      //   + 2^17 * waves per workgroup of the strips (1 ... 8) + 2^21 * their planes per chunk (0 = by box)
      if (value <= 0) { h->shell2_qw = 0; h->shell2_ww = 8; h->shell2_zcw = 0; h->shell2_ws = 6; h->shell2_zcs = 0; return 0; }
      const int qw = value % 128, ww = (value >> 7) % 8 + ((value >> 7) % 8 == 0 ? 8 : 0), zcw = (value >> 10) % 128;
      const int ws = (value >> 17) % 16, zcs = (value >> 21) % 128;
      if ((qw != 0 && qw < 3) || qw > 64 || ws > 8) break;
      h->shell2_qw = qw; h->shell2_ww = ww; h->shell2_zcw = zcw;
      h->shell2_ws = ws > 0 ? ws : 6; h->shell2_zcs = zcs;
      return 0;
    }
    case FDTD_OPT_FUSED_LB: if (value != 0 && value != 256 && value != 512 && value != 1024) break; h->fused_lb = value; return 0;
    default: break;
  }
  return fail(h, "fdtd_set_option: bad key/value %d/%d", key, value);
}

int fdtd_get_stats(FdtdSolver* h, FdtdStats* out) {
  if (!h || !out) return -1;
  *out = h->stats;
  out->tile_rows = h->rows_f;
  out->tile_zchunk = h->last_zc > 0 ? h->last_zc : h->zchunk_f;      // what the last sweep used
  out->tile_order = h->xcd_remap < 0 ? kTileRun : h->xcd_remap;
  out->placement = (h->placement_tried << 8) | h->placement_kept;
  out->placement_ms_first = h->placement_ms[0];
  out->placement_ms_kept = h->placement_ms[h->placement_kept];
  out->stream_overlap = h->stream_overlap;
  out->stream_retries = h->stream_retries;
  out->two_step_pairs = h->two_step_pairs;
  out->tblock_planes = h->tblock_used;
  out->graph_pairs = h->graph_pairs;
  out->reserved0 = h->graph_status;
  out->fused2_pairs = h->fused2_pairs;
  out->fused2_shape = h->fused2_pairs ? (h->twostep_w_used | (h->twostep_zc_used << 6)) : 0;
  out->shell_pairs = h->shell_pairs;
  out->shell2_pairs = h->shell2_pairs;
  out->fused2_off_reason = h->fused2_pairs ? 0 : (h->f2_off_reason ? h->f2_off_reason : h->f2_dyn_reason);
  out->disp_pairs = h->disp.pairs;
  out->single_step_reason = h->f2_dyn_reason;
  out->src_paged_pairs = (int32_t)std::min<long long>(h->spg.pairs, 0x7fffffff);
  out->struct_bytes = (int32_t)sizeof(FdtdStats);
  return 0;
}

int fdtd_get_seam_stats(FdtdSolver* h, FdtdSeamStats* out) {
  if (!h || !out) return -1;
  out->seam_deferred_pairs = h->seam_deferred_pairs;
  out->seam_flushes = h->seam_flushes;
  out->seam_pending = h->seam_pending ? 1 : 0;
  out->reserved = 0;
  out->seam_flush_ms = h->seam_flush_ms;
  return 0;
}

int fdtd_get_sweep_words(FdtdSolver* h, int64_t* out, int cap) {
  if (!h || (cap > 0 && !out)) return -1;
  const int n = (int)h->sweep_words.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = h->sweep_words[i];
  return n;
}

int fdtd_sweep_table(int64_t* out, int cap) {
  if (cap > 0 && !out) return -1;
  static const int64_t table[] = {
#define FDTD_F2_X(LBV, OV) FDTD_SWEEP_WORD(LBV, OV, 0),
      FDTD_F2_LIST_ALL(FDTD_F2_X)
#undef FDTD_F2_X
  };
  const int n = (int)(sizeof(table) / sizeof(table[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = table[i];
  return n;
}

}  // extern "C"
