/* fdtd_hip.h — C ABI of libfdtd_hip.so, the MI355X (gfx950) FDTD time-stepper.
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (flexcompute/tidy3d) has NO native interface for this path: its solver is a closed cloud
 * service reached through  tidy3d/web/api/webapi.py:49 run() -> :159 upload() -> :266 start()
 * -> :337 monitor() -> :631 load().  The functions below are what a local replacement of that
 * upload/start/monitor/load sequence binds through ctypes:
 *
 *   upload  (webapi.py:159, hdf5 of the Simulation)      -> fdtd_create + fdtd_set_* / fdtd_add_*
 *   start + monitor (webapi.py:266,:337; progress =
 *        (perc_done, field_decay), task_core.py:537)     -> fdtd_run + FdtdProgressFn
 *   load    (webapi.py:631, hdf5 of the monitor data)    -> fdtd_get_monitor / fdtd_get_field
 *   task status "diverged" (webapi.py:370)               -> FdtdStats.diverged
 *
 * Conventions
 *  - plain C; every function returns 0 on success, <0 on error; the message is available from
 *    fdtd_last_error() (thread-local for create, per-handle otherwise).
 *  - the caller owns every host buffer before and after a call (the library copies in/out
 *    synchronously); the library owns all device memory, streams and RCCL communicators.
 *  - one handle = one solve on one GPU (one z-slab of the domain in a multi-GPU run); calls on
 *    a handle are not re-entrant and must come from one host thread.
 *  - field arrays are [nz][ny][nx] C-ordered, x fastest, fp32 (ref monitor.py:35-36: 4 B real /
 *    8 B complex).  Yee staggering as in ref components/grid/grid.py:465-491.
 *  - component ids: 0..5 = Ex,Ey,Ez,Hx,Hy,Hz.
 */
#ifndef FDTD_HIP_H
#define FDTD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FdtdSolver FdtdSolver;

enum { FDTD_BC_PEC = 0, FDTD_BC_PMC = 1, FDTD_BC_PERIODIC = 2, FDTD_BC_NEIGHBOR = 3 };
enum { FDTD_MON_TIME = 0, FDTD_MON_DFT = 1, FDTD_MON_FLUX_TIME = 2 /* added by fdtd_add_flux_time_monitor only */,
       FDTD_MON_TIME_SPARSE = 3 /* added by fdtd_add_field_time_monitor only */,
       FDTD_MON_DFT_SPARSE = 4 /* added by fdtd_add_field_dft_monitor only */,
       FDTD_MON_DFT_LATTICE = 5 /* added by fdtd_add_lattice_dft_monitor only */ };
/* kernel variants of the two main update kernels (A/B-tested by bench.py --variant) */
/* AUTO = FUSED on one GPU (single-sweep E+H update, 48 B/cell-step), two-pass ZMARCH otherwise */
enum { FDTD_VARIANT_AUTO = 0, FDTD_VARIANT_SIMPLE = 1, FDTD_VARIANT_ZMARCH = 2, FDTD_VARIANT_FUSED = 3 };
enum { FDTD_FLAG_TIME_KERNELS = 1 };   /* bracket every main-kernel launch with hipEvents */

typedef struct FdtdConfig {
  int32_t nx, ny, nz;      /* cells of THIS rank's slab (PML cells included)                    */
  int32_t bc[6];           /* xmin,xmax,ymin,ymax,zmin,zmax: FDTD_BC_*; NEIGHBOR only on z faces */
  int32_t device;          /* HIP device ordinal                                                */
  int32_t variant;         /* FDTD_VARIANT_*                                                    */
  int32_t flags;           /* FDTD_FLAG_*                                                       */
  int32_t z_chunk;         /* planes marched per workgroup (0 = default)                        */
  float   ch;              /* dt / mu0: H-update coefficient                                    */
  int32_t reserved[6];
} FdtdConfig;

typedef struct FdtdStats {
  int64_t steps_done;
  int32_t diverged;          /* NaN/Inf seen in the field-energy reduction                       */
  int32_t stopped_early;     /* shutoff reached                                                  */
  double  field_decay;       /* last W / max W,  W = sum|E|^2 + (mu0/eps0) sum|H|^2              */
  double  run_ms;            /* hipEvent time of the last fdtd_run (whole step loop)             */
  double  h_kernel_ms;       /* with FDTD_FLAG_TIME_KERNELS: summed durations of the main H ...  */
  double  e_kernel_ms;       /* ... and E update kernels in the last fdtd_run                    */
  int64_t h_kernel_launches;
  int64_t e_kernel_launches;
  int64_t device_bytes;      /* device memory held by the handle                                 */
  double  fused_kernel_ms;   /* ... and of the fused E+H sweep                                   */
  int64_t fused_kernel_launches;
  int32_t tile_rows;         /* tile shape of the fused sweep in use (after autotuning)           */
  int32_t tile_zchunk;
  int32_t tile_order;        /* 1 = XCD-aware tile order, 0 = plain (chosen by timing both on the first large sweep) */
  int32_t placement;         /* placement probe of the field arrays: (candidates timed << 8) | index kept (0 = the first allocations) */
  float   placement_ms_first;/* three probe sweeps on the first allocations ...                 */
  float   placement_ms_kept; /* ... and on the set that was kept (0 when the probe did not run) */
  int32_t stream_overlap;    /* the engine's two streams: 1 = measured to run concurrently, 0 = not probed yet (no run used
                                both), -1 = they serialised on every attempt (shared hardware queue): ONE stream is used */
  int32_t stream_retries;    /* fresh second streams created until two overlapped                */
  int32_t comm_ranks;        /* ncclCommCount of the halo communicator (0 = none)                */
  int32_t comm_rank;         /* ncclCommUserRank                                                 */
  int64_t two_step_pairs;    /* step pairs advanced by the slab-interleaved two-step schedule (FDTD_OPT_TBLOCK) in the last fdtd_run */
  int32_t tblock_planes;     /* its slab thickness in planes (0 = schedule off)                  */
  int32_t reserved0;         /* graph capture diagnostics: 0 = none attempted, 1 = captured, < 0 = -(100 stage + hipError) */
  int64_t graph_pairs;       /* step pairs replayed as captured hipGraphs in the last fdtd_run (FDTD_OPT_GRAPH) */
  int64_t fused2_pairs;      /* step pairs advanced by the two-steps-per-sweep kernel in the last fdtd_run (FDTD_OPT_TWOSTEP) */
  int64_t fused2_shape;      /* its tile shape: waves per workgroup | planes per chunk << 6 (0 = no pair was taken) */
  int64_t shell_pairs;       /* of those: pairs of a CPML-walled grid — the two-step sweep over the bulk, the shell (CPML slabs + collar)
                                as two single steps beside it on the second stream (FDTD_OPT_SHELL_PAIRS) */
  double  shell_kernel_ms;   /* with FDTD_FLAG_TIME_KERNELS: summed durations of the shell launches (they overlap the bulk sweep) */
  int64_t shell_kernel_launches;
  int64_t shell2_pairs;      /* of those: pairs whose shell went out as shell2_step_kernel launches — two steps per sweep with the CPML
                                recursions carried through both — instead of two single steps (FDTD_OPT_SHELL2) */
  int32_t fused2_off_reason; /* why the last fdtd_run took NO step pairs: FDTD_F2_OFF_* (0 = it took some, or had no chance to: < 2 steps) */
  int32_t struct_bytes;      /* sizeof(FdtdStats) of the library that filled this in (a binding checks it against its own layout) */
  int64_t disp_pairs;        /* of fused2_pairs: pairs that advanced the dispersive (ADE) cells themselves (FDTD_OPT_DISP; round 6) */
  int32_t single_step_reason;/* a run that took pairs AND single steps: the last FDTD_F2_OFF_* that kept a step from opening a pair because of its
                                sources (a TFSF box / mode plane while it injects ...); 0 = none (single steps then are record / decay-check /
                                odd-count steps) */
  int32_t src_paged_pairs;   /* of fused2_pairs: pairs that carried paged source terms (FDTD_OPT_SRC_PAGED; round 6) */
  double  seam_kernel_ms;    /* with FDTD_FLAG_TIME_KERNELS: summed durations of seam_kernel behind the two-step sweeps (until round 6 they
                                were part of fused_kernel_ms, which now brackets the sweep alone — what rocprofv3 reports for the kernel) */
  int64_t seam_kernel_launches;
} FdtdStats;

/* Deferred seam repair of the last fdtd_run (FDTD_OPT_SEAM_DEFER).  Its own structure: the layout of FdtdStats stays what bindings built
 * against earlier headers expect. */
typedef struct FdtdSeamStats {
  int64_t seam_deferred_pairs; /* of fused2_pairs: pairs whose seam_kernel left its values in the compact repair array for the next pair's
                                  sweep instead of storing them into the fields */
  int64_t seam_flushes;        /* launches of seam_flush_kernel: a repair array scattered into the fields because something other than the
                                  expected plain pair was about to read them */
  int32_t seam_pending;        /* 1: the current set's seam columns are stale (never, once fdtd_run has returned) */
  int32_t reserved;
  double  seam_flush_ms;       /* with FDTD_FLAG_TIME_KERNELS: summed durations of the flushes (not part of FdtdStats.seam_kernel_ms, which
                                  keeps counting every seam_kernel launch, deferred or not) */
} FdtdSeamStats;

/* FdtdStats.fused2_off_reason: what keeps a run on single steps (the first reason found) */
enum { FDTD_F2_OFF_NONE = 0,
       FDTD_F2_OFF_DISABLED = 1,          /* FDTD_OPT_TWOSTEP = 0 (or another schedule was asked for) */
       FDTD_F2_OFF_TOO_SMALL = 2,         /* grids below 2^20 cells are bound by launches, not by bytes */
       FDTD_F2_OFF_COMM = 3,              /* z-slab rank (RCCL communicator): ghost planes are exchanged every step */
       FDTD_F2_OFF_PML = 4,               /* CPML present and shell pairs not possible: switched off, slab-kernel CPML asked for,
                                             layers too thick for the grid, absorber layers on another axis */
       FDTD_F2_OFF_ADE = 5,               /* dispersive media whose cells are not confined to a few plane ranges along z (their planes take single
                                             steps as z holes of the bulk; what is left must be worth a two-step launch), or with absorber layers */
       FDTD_F2_OFF_TFSF = 6,              /* a TFSF box while it injects (a plane wave's injection PLANE is a z hole of the bulk: pairs) */
       FDTD_F2_OFF_BOUNDARY = 7,          /* periodic / Bloch faces, PMC on a plus face, rows not a multiple of 4 cells */
       FDTD_F2_OFF_H_SOURCE_ABSORBER = 8, /* magnetic point sources together with absorber layers */
       FDTD_F2_OFF_SEAM_SOURCE = 9,       /* an H_y / H_z source node in the column left of a seam between 256-cell x tiles */
       FDTD_F2_OFF_SOURCES = 10,          /* while they inject: more than 256 source nodes that are not confined to a few planes along z (a mode plane /
                                             current sheet normal to z is a z hole of the bulk: pairs), or H-side nodes without room for their table */
       FDTD_F2_OFF_VARIANT = 11,          /* the run is not on the fused sweep at all (two-pass kernels) */
       FDTD_F2_OFF_SHELL = 12,            /* CPML shell too large a part of the grid for shell pairs to pay (cost model, fdtd_capi.hip shell_why_not) */
       FDTD_F2_OFF_MEMORY = 13,           /* no room for the third field set that shell pairs / slab pairs keep the middle step in (+ 50 % field memory) */
       FDTD_F2_OFF_WIDE_TABLE = 14,       /* more than 1023 media (16-bit indices, two words per cell): the single-step sweep reads them, the two-step and shell sweeps do not */
       FDTD_F2_OFF_MODULATION = 15,       /* time-modulated media (fdtd_add_modulation): their list kernels run in front of and behind every single step */
       FDTD_F2_OFF_CONFORMAL = 16,        /* PEC-conformal boundaries (fdtd_add_pec_conformal): their list kernel runs in front of every single step */
       FDTD_F2_OFF_NONLINEAR = 17 };      /* Kerr media (fdtd_add_nonlinear): their fixed-point iterations follow every single step */

/* progress callback: (step, time [s], field_decay) -> non-zero aborts the run (Ctrl-C path).
 * Mirrors the (perc_done, field_decay) pair the cloud reports (ref web/core/task_core.py:537). */
typedef int (*FdtdProgressFn)(int64_t step, double time, double field_decay, void* user);

const char* fdtd_last_error(const FdtdSolver* h);   /* h may be NULL: error of the last create */
int  fdtd_device_count(void);

/* Near -> far projection, the integration step on the device (ref components/field_projection.py:360-368
 * `integrate_2d` and :370 `_far_fields_for_surface`).  For one surface of a projection
 * monitor at one frequency: the equivalent currents J_u, J_v, M_u, M_v on the (u, v) lattice of the surface
 * (`currents`: [4][n_u][n_v] complex as (re, im) pairs of doubles; coordinates u[n_u], v[n_v] relative to the
 * monitor's local origin, w0 = the surface's coordinate along its normal; wu, wv = the trapezoid weights of
 * np.trapz, 1 for a single point) are integrated against exp(-i k r_hat . r') for n_dir directions given by their
 * cosines (r_u, r_v, r_w) along u, v and the normal; k = k_re + i k_im in the projection medium.
 * out[n_dir][4][2] = the four integrals (re, im) per direction.  Returns 0, or -1 with fdtd_last_error(NULL). */
int  fdtd_far_field(int device, int n_u, int n_v, const double* u, const double* v, const double* wu, const double* wv,
                    const double* currents, double w0, double k_re, double k_im, int n_dir, const double* r_u,
                    const double* r_v, const double* r_w, double* out);

/* Exact projection (far_field_approx=False; ref components/field_projection.py:831-1010), the integration step on the
 * device: the sibling of fdtd_far_field for observation POINTS at a finite distance.  Same surface description (one
 * surface, one frequency: u, v, wu, wv, currents [4][n_u][n_v], w0, k); n_pts points by their coordinates (p_u, p_v, p_w)
 * in the same local frame (along u, v and the normal, relative to the monitor's local origin).  With Rv = p - r',
 * R = |Rv|, Rh = Rv / R, G = exp(i k R) / (4 pi R), G1 = G (i k - 1/R), G2 = G1 (i k - 1/R) + G / R^2 and, per current
 * type F in {J, M} (F_w = 0), rd = Rh_u F_u + Rh_v F_v:
 *   I_F[a] = sum wu wv [G F_a + (Rh_a rd G2 + (F_a - Rh_a rd) G1 / R) / k^2],  C_F[a] = sum wu wv G1 (Rh x F)_a,  a in (u, v, w)
 * (the cross product of a right-handed (u, v, w)).  out[n_pts][12][2] = I_J, I_M, C_J, C_M (re, im), all in fp64; the
 * caller forms E = i w mu0 I_J - C_M, H = i w eps0 eps I_M + C_J.  A point on a lattice node gives non-finite values.
 * n_pts == 0 returns 0 without touching out.  Returns 0, or -1 with fdtd_last_error(NULL). */
int  fdtd_near_field(int device, int n_u, int n_v, const double* u, const double* v, const double* wu, const double* wv,
                     const double* currents, double w0, double k_re, double k_im, int n_pts, const double* p_u,
                     const double* p_v, const double* p_w, double* out);
/* The number of lattice chunks fdtd_near_field cuts an n_u x n_v lattice into for n_pts points (a function of n_pts and
 * n_u * n_v alone: csrc/fdtd_near_field.hpp); -1 on a bad argument.  Needs no device. */
int  fdtd_near_field_chunks(int n_pts, int n_u, int n_v);

/* One solve = one handle.  Stands in for SimulationTask.create + upload_simulation of the cloud
 * path (ref web/api/webapi.py:219,237; web/core/task_core.py:121); the grid size is
 * Simulation.grid.num_cells incl. the PML cells (ref simulation.py:4296, grid_spec.py:114-137),
 * the face codes come from Simulation.boundary_spec (ref boundary.py:732; a PEC wall backs every
 * PML, CHANGELOG.md:1290), ch = Simulation.dt / MU_0 (ref simulation.py:4194, constants.py:21). */
int  fdtd_create(const FdtdConfig* cfg, FdtdSolver** out);
/* ref web/api/webapi.py delete(): releases every device resource of the task */
void fdtd_destroy(FdtdSolver* h);

/* 1/primal and 1/dual step vectors of one axis (length = n cells of that axis of this slab;
 * ref grid.py:393-417).  axis 0,1,2 = x,y,z.  For z, n may also be nz + 2: then entry 0 and
 * n-1 are the values of the planes just below / above the slab (needed by the fused sweep on a
 * z-slab of a non-uniform grid); with n == nz they are derived from the boundary condition. */
int fdtd_set_steps(FdtdSolver* h, int axis, const float* inv_primal, const float* inv_dual, int n);

/* material table (index 0 = PEC: ca = cb = 0) and, optionally, the staircased material index
 * volumes mat[3][nz][ny][nx] (uint8, one per E component, ref simulation.py:1135-1241).
 * Without fdtd_set_material every cell uses entry 1.  (Ca, Cb) follow from Medium.permittivity /
 * conductivity (ref medium.py:1499, :1016-1038) or the pole-residue form (ref medium.py:2739). */
int fdtd_set_media(FdtdSolver* h, const float* ca, const float* cb, int n_media);   /* n_media <= 1024 */
int fdtd_set_material(FdtdSolver* h, const uint8_t* mat, size_t bytes);
/* the same with 16-bit indices mat[3][nz][ny][nx] (count = 3 nz ny nx entries): more than 255 media (the
 * reference allows 65,530 structures, ref components/scene.py:52; the device packs three 10-bit indices
 * into one 32-bit word per cell, so 1023 distinct media per simulation) — what sub-pixel averaging and
 * CustomMedium need to quantise permittivity in 0.2 % steps */
int fdtd_set_material16(FdtdSolver* h, const uint16_t* mat, size_t count);

/* CPML tables of one axis, each of length n (identity outside the slabs); the slab index ranges
 * are derived from n_lo/n_hi = Simulation.num_pml_layers (ref simulation.py:1002) and the profile
 * from PMLParams (ref boundary.py:195-254; sampling positions ref plugins/mode/derivatives.py:
 * 174-197; formulas in tidy3d_amd/coeffs.py).  On a z-slab the host passes slab-local tables. */
int fdtd_set_pml(FdtdSolver* h, int axis, int n_lo, int n_hi,
                 const float* kinv_e, const float* b_e, const float* c_e,
                 const float* kinv_h, const float* b_h, const float* c_h, int n);

/* PMC on the PLUS face of an axis (ref boundary.py:45 PMCBoundary; the min face is FDTD_BC_PMC in FdtdConfig.bc).  The host
 * lays the axis out with two ghost cells beyond the wall (its plus face declared FDTD_BC_PEC: plain truncation) and names the
 * wall's cell-boundary index, wall == n_cells(axis) - 2; the library refreshes the mirror images beyond the wall at the
 * start of every step (tangential E and normal H even, normal E and tangential H odd).  wall < 0 switches it off.
 * One GPU (not on z-slabs, not with fdtd_run_bloch). */
int fdtd_set_mirror_plus(FdtdSolver* h, int axis, int wall);

/* Absorber layers of one axis (ref boundary.py:427-476 Absorber, :166-192 AbsorberParams; layer
 * counts = Simulation.num_pml_layers, ref simulation.py:1002): per-step damping factors of length n
 * (1 outside the layers), fb sampled at the cell boundaries, fc at the cell centres; the layers are
 * [0, n_lo) and [n - n_hi, n).  Every component inside them is multiplied once per step by the
 * product of its three axis factors (tidy3d_amd/coeffs.py damping_tables).  On a z-slab the host
 * passes slab-local tables and counts. */
int fdtd_set_absorber(FdtdSolver* h, int axis, int n_lo, int n_hi, const float* fb, const float* fc, int n);

/* pole-residue ADE group: the cells (linear index k*ny*nx + j*nx + i within the slab) of E
 * component `comp` filled with one dispersive medium; kap/bet are n_poles complex pairs
 * (re,im interleaved), cc the memory-term coefficient (ref medium.py:2900-2913). */
int fdtd_add_ade(FdtdSolver* h, int comp, int64_t n_cells, const uint32_t* cell_index,
                 int n_poles, const float* kap, const float* bet, float cc);

/* fully anisotropic bodies (ref tidy3d medium.py:5058 FullyAnisotropicMedium): the off-diagonal coupling of E component `comp`
 * at n nodes.  The sweep advances every component with the diagonal of eps^-1 (table media); behind it
 *     E_comp[cell[i]] += sum_{s<8} w_new[8i+s] * Eb^{n+1}[nbr[8i+s]] - w_old[8i+s] * Eb^n[nbr[8i+s]],
 * slots 0-3: component (comp+1)%3, slots 4-7: (comp+2)%3; nbr = 0xFFFFFFFF: no node (weight ignored).  The host forms
 * w_new = (dt/eps0) g / Cb(nbr), w_old = w_new * Ca(nbr) (tidy3d_amd/spec.py AnisoSet).  Single steps only; not on z-slabs. */
int fdtd_add_aniso(FdtdSolver* h, int comp, int64_t n_nodes, const uint32_t* cell_index, const uint32_t* nbr_index,
                   const float* w_new, const float* w_old);
/* the same list for a pair of handles advanced by fdtd_run_bloch (give both handles the same lists, in the same order).  A slot whose
 * neighbour lies one period away across a periodic / Bloch face names the real node on the far side (not a ghost cell; its Ca / Cb
 * in the weights) and carries a wrap code: bits 2a, 2a+1 = the period crossed along axis a (0 = none, 1 = +1 beyond the upper
 * face, 2 = -1 beyond the lower face).  fdtd_run_bloch multiplies that neighbour's term by exp(i sum_a s_a phase[a]) and so mixes
 * the two parts; fdtd_run ignores the codes (phase 0). */
int fdtd_add_aniso_bloch(FdtdSolver* h, int comp, int64_t n_nodes, const uint32_t* cell_index, const uint32_t* nbr_index,
                         const float* w_new, const float* w_old, const uint8_t* wrap);

/* time-modulated media (ref tidy3d components/time_modulation.py ModulationSpec on a Medium): n nodes of E component `comp` whose
 * permittivity and / or conductivity follow
 *     eps(t) = eps_bar + Re[d_eps exp(-i w_eps t)],    sigma(t) dt / (2 eps0) = s_bar + Re[d_s exp(-i w_sig t)]
 * (d_eps, d_s: n complex values, re / im interleaved, the time modulation's amplitude and phase folded in; d_s = d_sigma dt / (2 eps0)).
 * The sweep advances these nodes with their static table medium, E_lin = Ca E^n + Cb K; at the end of the E phase of step n the
 * library replaces that by
 *     E^{n+1} = alpha E^n + beta (E_lin - ca E^n),   alpha = (eps^n - s) / (eps^{n+1} + s),   beta = (eps_bar + s_bar) / (eps^{n+1} + s),
 *     eps^n = eps(n dt),  eps^{n+1} = eps((n + 1) dt),  s = sigma((n + 1/2) dt) dt / (2 eps0)
 * which is (D^{n+1} - D^n) / dt + sigma^{n+1/2} (E^{n+1} + E^n) / 2 = K with D = eps0 eps(t) E.  ca, eps_bar, s_bar: the node's own
 * table coefficient Ca and the host's eps_bar = dt / (eps0 Cb) * 2 / (1 + Ca), s_bar = eps_bar (1 - Ca) / (1 + Ca).
 * omega_eps, omega_sigma: the PHASE ADVANCE PER TIME STEP in radians, 2 pi f dt, of the two modulations (the library forms the phase
 * of step n in double from the step count).  Cell indexing as in fdtd_add_aniso; a node is listed at most once per component; eps_bar +
 * s_bar must exceed |d_eps| + |d_s|.  A handle with such a list takes single steps only (FDTD_F2_OFF_MODULATION), no captured graphs,
 * no slab-interleaved schedule, and is refused on z-slabs (FDTD_BC_NEIGHBOR faces, fdtd_comm_init).  fdtd_run_bloch: give both handles
 * the same lists — the update is linear with real coefficients, each part is patched on its own. */
int fdtd_add_modulation(FdtdSolver* h, int comp, int64_t n_nodes, const uint32_t* cell_index, const float* ca, const float* eps_bar,
                        const float* s_bar, const float* d_eps /* [2 n] */, const float* d_s /* [2 n] */, double omega_eps,
                        double omega_sigma);

/* PEC-conformal boundaries (ref tidy3d components/subpixel_spec.py PECConformal; the Dey-Mittra scheme): n faces of H component
 * `comp` (3..5) cut by a PEC surface.  In front of the H update of every step the library adds
 *     H_comp[cell_index[i]] += sum_{k = 0..3} d[k n + i] E_k[nbr_index[k n + i]]        (E^n; summed in the order k = 0..3)
 * with c = comp - 3, a1 = (c + 1) % 3, a2 = (c + 2) % 3: slots k = 0, 1 read E_a2 (one node up along a1, the face's own index),
 * k = 2, 3 read E_a1 (one node up along a2, the face's own index); nbr_index 0xFFFFFFFF = no node.  d[k] = -(dt / mu0) s_k
 * (l_k / A - 1) * inv_step_k with s = (+, -, -, +), l_k the free fraction of the edge, A the (clamped) free fraction of the face and
 * inv_step_k the float32 inverse PRIMAL step of fdtd_set_steps along a1 (k = 0, 1) / a2 (k = 2, 3): the sweep applies the same sum
 * with l_k / A = 1.  nbr_index and d are [4][n] (structure of arrays).  Cell indexing as in fdtd_add_aniso; a face is listed at most
 * once per component.  A handle with such a list takes single steps only (FDTD_F2_OFF_CONFORMAL), no captured graphs, no
 * slab-interleaved schedule, and is refused on z-slabs (FDTD_BC_NEIGHBOR faces, fdtd_comm_init).  fdtd_reset keeps the lists.
 * fdtd_run_bloch: give both handles the same lists (the correction is linear with real coefficients). */
int fdtd_add_pec_conformal(FdtdSolver* h, int comp, int64_t n_faces, const uint32_t* cell_index, const uint32_t* nbr_index,
                           const float* d);

/* Kerr media (ref tidy3d components/medium.py NonlinearSpec / NonlinearSusceptibility): n nodes of E component `comp` with the
 * instantaneous third-order response D = eps0 (eps_bar + chi3 I) E, I = |E|^2 at the node:
 *     I = E_a^2 + (mean of the four surrounding E_b nodes)^2 + (mean of the four surrounding E_c nodes)^2,   b = a + 1, c = a + 2 (cyclic)
 * nbr_index is [8][n] (structure of arrays): slots 0..3 the E_b nodes, 4..7 the E_c nodes, in the order of fdtd_add_aniso's slots;
 * 0xFFFFFFFF = no node (beyond a PEC / PMC wall): it contributes 0 to its mean of four.  The sweep advances these nodes with their
 * static table medium, E_lin = Ca E^n + Cb K; at the end of the E phase the library solves
 *     (D^{n+1} - D^n) / dt + sigma (E^{n+1} + E^n) / 2 = K
 * by num_iters Jacobi fixed-point iterations, E^(0) = E_lin,
 *     E^(m) = alpha_m E^n + beta_m (E_lin - ca E^n),   alpha_m = (eps_bar + chi3 I^n - s_bar) / (eps_bar + chi3 I^(m-1) + s_bar),
 *                                                      beta_m  = (eps_bar + s_bar) / (eps_bar + chi3 I^(m-1) + s_bar)
 * where I^(m-1) is formed from the fields as iteration m - 1 left them, every listed node of all three components before any is
 * overwritten.  ca, eps_bar, s_bar: the node's own table coefficient and the host's eps_bar, s_bar of fdtd_add_modulation; ca must be
 * (eps_bar - s_bar) / (eps_bar + s_bar) to 1e-5 (the library evaluates the iterate as E_lin + chi3 (I^n E^n - I^(m-1) E_lin) /
 * (eps_bar + s_bar + chi3 I^(m-1)), which is the same number and the table update, bit for bit, where chi3 = 0).  Cell indexing as
 * in fdtd_add_aniso; one list per component, a node at most once in it; 1 <= num_iters <= 64, the same for all lists of a handle.
 * A handle with such a list takes single steps only (FDTD_F2_OFF_NONLINEAR), no captured graphs, no slab-interleaved schedule, no
 * paged ADE memory terms, and is refused on z-slabs (FDTD_BC_NEIGHBOR faces, fdtd_comm_init), by fdtd_run_bloch (the update is not
 * linear: the two parts cannot be patched separately) and together with fdtd_add_modulation lists.  fdtd_reset keeps the lists. */
int fdtd_add_nonlinear(FdtdSolver* h, int comp, int64_t n_nodes, const uint32_t* cell_index, const uint32_t* nbr_index /* [8][n] */,
                       const float* ca, const float* eps_bar, const float* s_bar, const float* chi3, int num_iters);

/* current source: F[comp[p]][index[p]] += w_re[p]*Re(wave[n]) - w_im[p]*Im(wave[n]);
 * E components use wave_e (sampled at t_n + dt/2), H components wave_h (t_n);
 * waves are n_steps complex values (re,im interleaved)  (ref source.py:174-193, :543-632). */
int fdtd_add_point_source(FdtdSolver* h, int64_t n_points, const int32_t* comp,
                          const uint32_t* cell_index, const float* w_re, const float* w_im,
                          int64_t n_steps, const float* wave_e, const float* wave_h);

/* total-field/scattered-field source driven by a 1-D auxiliary grid (ref source.py:1204-1257);
 * semantics documented at tidy3d_amd/spec.py TfsfSpec.  aux indices refer to e1 (h_corr) and
 * h1 (e_corr). */
int fdtd_add_tfsf(FdtdSolver* h, int n_aux, const float* ae, const float* be,
                  const float* ah, const float* bh, int src_cell,
                  int64_t n_steps, const float* wave,
                  int64_t n_e, const int32_t* e_comp, const uint32_t* e_index, const float* e_w,
                  const int32_t* e_aux,
                  int64_t n_h, const int32_t* h_comp, const uint32_t* h_index, const float* h_w,
                  const int32_t* h_aux);

/* monitor over the Yee index box [lo, hi) of this slab.  steps: sorted time-step indices on
 * which it records.  DFT monitors: nf frequencies and phase tables [n_rec][nf] complex
 * (re,im interleaved) for E (t_n) and H (t_n + dt/2) samples (ref monitor.py:363-403,
 * time.py:95-105).  Returns the monitor id (>= 0) or <0. */
int fdtd_add_monitor(FdtdSolver* h, int kind, int n_comps, const int32_t* comps,
                     const int32_t lo[3], const int32_t hi[3],
                     int64_t n_rec, const int64_t* steps,
                     int nf, const float* phase_e, const float* phase_h);
/* FDTD_MON_FLUX_TIME (ref monitor.py FluxTimeMonitor, one planar surface): the flux through a plane normal to `axis` at every step of
 * `steps`, reduced on the device — the result is float[n_rec], and the device holds a ring of records instead of n_rec of them.
 * The monitor records like the FDTD_MON_TIME monitor of the box [lo, hi) with the components E_t1, E_t2, H_t1, H_t2, t1 = axis + 1,
 * t2 = axis + 2 (cyclic), in every schedule, into a staging buffer of R = staging_bytes / (record bytes) records (at least 2, at most
 * n_rec; staging_bytes <= 0: 32 MiB), slot = record index mod R; when the ring is full, at the end of fdtd_run and in front of
 * fdtd_get_monitor one launch turns every complete record of every such monitor into
 *     flux[rec] = sign * sum over nodes (E_t1 H_t2 - E_t2 H_t1) * weight(node)        (fp32, fixed summation order, no atomics)
 * on the n_nodes[0] x n_nodes[1] x n_nodes[2] primal nodes of the surface (n_nodes[axis] == 1).  Each component is colocated to a node by
 * separable linear interpolation: tap_index / tap_weight hold, axis after axis (x, y, z), [4 components][n_nodes[a]][2] taps — the index
 * into the box along that axis and its weight; a tap of weight 0 is not read, every other index must lie inside the box.
 * weight(node) = wu[i_u] * wv[i_v], u < v the two tangential axes (wu[n_nodes[u]], wv[n_nodes[v]]).
 * Added between runs, the steps already done are skipped (their entries stay 0 until fdtd_reset, after which it records them all).
 * Refused on z-slab handles (FDTD_BC_NEIGHBOR faces, fdtd_comm_init); fdtd_run_bloch refuses handles that carry one.
 * Returns the monitor id (>= 0) or <0. */
int fdtd_add_flux_time_monitor(FdtdSolver* h, int axis, float sign, const int32_t lo[3], const int32_t hi[3],
                               int64_t n_rec, const int64_t* steps, const int32_t n_nodes[3],
                               const int32_t* tap_index, const float* tap_weight,
                               const float* wu, const float* wv, int64_t staging_bytes);
/* FDTD_MON_TIME_SPARSE (ref monitor.py FieldTimeMonitor with interval_space / colocate): the components `comps` on the nodes the
 * monitor keeps, at every step of `steps`, gathered on the device — the result is float [n_rec][component][n_z][n_y][n_x] with the
 * node counts of each component its own (n_targets[3 * c + a], a = x, y, z; the components follow one another inside a record), and
 * the device holds a ring of records of the box [lo, hi) instead of n_rec of them.  The monitor records like the FDTD_MON_TIME monitor
 * of that box in every schedule, into a staging buffer of R = staging_bytes / (record bytes) records (at least 2, at most n_rec;
 * staging_bytes <= 0: 32 MiB), slot = record index mod R; when the ring is full, at the end of fdtd_run and in front of fdtd_get_monitor
 * one launch per monitor forms, for every complete record, component and kept node,
 *     out = sum over the 2 x 2 x 2 taps of wx wy wz raw[jz][jy][jx]        (separable: x, then y, then z; fp32)
 * tap_index / tap_weight hold, component after component and inside a component axis after axis (x, y, z), [n_targets][2] taps — the
 * index into the box along that axis and its weight; a tap of weight 0 is not read, every other index must lie inside the box.
 * Added between runs, the steps already done are skipped (their records stay 0 until fdtd_reset, after which it records them all).
 * Refused on z-slab handles (FDTD_BC_NEIGHBOR faces, fdtd_comm_init); fdtd_run_bloch refuses handles that carry one.
 * Returns the monitor id (>= 0) or <0. */
int fdtd_add_field_time_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                                int64_t n_rec, const int64_t* steps, const int32_t* n_targets,
                                const int32_t* tap_index, const float* tap_weight, int64_t staging_bytes);
/* FDTD_MON_DFT_SPARSE (ref monitor.py FieldMonitor with interval_space / colocate): the running DFT of the components `comps` on the
 * nodes the monitor keeps — the result is complex64 [nf][component][n_z][n_y][n_x], the node counts of each component its own
 * (n_targets[3 * c + a], a = x, y, z; the components follow one another inside a frequency), and the device holds these accumulators
 * and nothing of the box [lo, hi).  The monitor records like the FDTD_MON_DFT monitor of that box in every schedule (E at step n with
 * phase_e, H at n + 1/2 with phase_h, both [n_rec][nf] complex64; inside step pairs from the sweep's copy of the middle step); at
 * every record each sample is colocated onto the kept nodes first,
 *     v = sum over the 2 x 2 x 2 taps of wx wy wz F[jz][jy][jx]           (separable: x, then y, then z; fp32)
 *     acc[f][node] += v * phase[rec][f]
 * with the tap tables of fdtd_add_field_time_monitor (same layout, same checks: a tap of weight 0 is not read, every other index
 * must lie inside the box).  Added between runs, the steps already done are skipped: it accumulates from then on (fdtd_reset: from
 * step 0).  Refused on z-slab handles (FDTD_BC_NEIGHBOR faces, fdtd_comm_init); fdtd_run_bloch refuses handles that carry one.
 * Returns the monitor id (>= 0) or <0. */
int fdtd_add_field_dft_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                               int64_t n_rec, const int64_t* steps, const int32_t* n_targets,
                               const int32_t* tap_index, const float* tap_weight, int nf, const float* phase_e, const float* phase_h);
/* FDTD_MON_DFT_LATTICE (ref monitor.py FieldProjectionAngleMonitor / CartesianMonitor / KSpaceMonitor: one surface of a projection
 * monitor): the running DFT of the components `comps` on the surface's sampling lattice — everything as FDTD_MON_DFT_SPARSE (the result
 * complex64 [nf][component][n_z][n_y][n_x], fdtd_get_monitor and fdtd_get_monitor_bytes, the schedules, adding between runs, fdtd_reset,
 * the refusals), but with n_taps = 4 taps per node and axis, tables [n_targets][n_taps] per component and axis: a lattice point lies
 * between two colocated nodes with two Yee taps each, in the order node j tap 0, node j tap 1, node j + 1 tap 0, node j + 1 tap 1,
 *     v = sum over the 4 x 4 x 4 slots of wx wy wz F[jz][jy][jx]          (separable: x, then y, then z; fp32; the slots in table order,
 *                                                                        duplicates not merged; a slot of weight 0 is neither read nor added)
 * The lanes of a wave run along the first axis on which a component keeps more than one node (csrc/fdtd_lattice_dft.hpp): the result
 * layout does not depend on it.  Any other n_taps is refused.  Returns the monitor id (>= 0) or <0. */
int fdtd_add_lattice_dft_monitor(FdtdSolver* h, int n_comps, const int32_t* comps, const int32_t lo[3], const int32_t hi[3],
                                 int64_t n_rec, const int64_t* steps, const int32_t* n_targets, int n_taps /* 4 */,
                                 const int32_t* tap_index, const float* tap_weight, int nf, const float* phase_e, const float* phase_h);
/* The power through a surface from its lattice accumulators, reduced on the device (ref monitor.py DirectivityMonitor: the radiated
 * power a directivity is normalised by; csrc/fdtd_lattice_flux.hpp).  `monitor_id`: a lattice DFT monitor that holds the four
 * components tangential to `axis`; a surface is one monitor here, a closed box is six calls.
 * fdtd_set_lattice_flux_weights, once per monitor, with the plan: the orientation `sign` of the surface and the integration weights
 * along the three axes — n[a] of them, as many as the monitor keeps nodes along a, one ([1]) along the normal.
 * fdtd_lattice_flux, after a run:
 *     out[k] = sign * sum over the lattice of w0 w1 w2 * 0.5 Re(E x conj H) . n_axis,   k < nf, double,
 * from the accumulators as they stand (before any source normalisation), one workgroup of 256 per frequency, fp64, a fixed order
 * of summation, no atomics.  Both refuse, with the handle's error string and without a launch: an id that is no lattice DFT
 * monitor, z-slab handles, the handles of an fdtd_run_bloch pair; fdtd_lattice_flux a monitor without weights.  Return 0 or <0. */
int fdtd_set_lattice_flux_weights(FdtdSolver* h, int monitor_id, int axis, double sign, const int32_t n[3], const double* w0,
                                  const double* w1, const double* w2);
int fdtd_lattice_flux(FdtdSolver* h, int monitor_id, double* out /* [nf] */);
/* time: float [n_rec][n_comps][bz][by][bx];  dft: complex64 [nf][n_comps][bz][by][bx];  flux-time: float [n_rec];
 * sparse field-time: float [n_rec][sum over the components of their kept nodes];
 * sparse DFT, lattice DFT: complex64 [nf][sum over the components of their kept nodes] */
int fdtd_get_monitor(FdtdSolver* h, int monitor_id, void* host, size_t bytes);
/* device memory a monitor holds, as allocated: out[0] = all of it, out[1] = its record buffer (flux-time, sparse field-time: the staging ring),
 * out[2] = the reduced series of a flux-time monitor / the gathered array of a sparse field-time monitor / the accumulators of a
 * sparse or lattice DFT monitor, nf x kept nodes x 8 B (which holds no records: out[1] = 0) (else 0),
 * out[3] = tables (phase tables; taps, weights, per-tile partial sums) */
int fdtd_get_monitor_bytes(FdtdSolver* h, int monitor_id, int64_t out[4]);

/* whole-volume field access [nz][ny][nx] (tests, benchmarks; a checkpoint is fdtd_get_state / fdtd_set_state below: the fields are
 * not the whole state); the reference exposes fields only through monitors (ref monitor.py:363), so this has no cloud counterpart */
int fdtd_set_field(FdtdSolver* h, int comp, const float* host, size_t bytes);
int fdtd_get_field(FdtdSolver* h, int comp, float* host, size_t bytes);

/* field-decay / shutoff: evaluate W = sum|E|^2 + (mu0/eps0) sum|H|^2 over the slab every `every` steps
 * (fixed-order reduction: bitwise repeatable); stop when W falls below shutoff * max W after step
 * `ref_step` (ref simulation.py:2089-2096 shutoff, "field decay" of web/core/task_core.py:537).
 * every = 0 disables.  A non-finite W ends the run with FdtdStats.diverged (ref sim_data.py:909). */
int fdtd_set_shutoff(FdtdSolver* h, int every, double shutoff, int64_t ref_step);

/* z-slab decomposition over RCCL (one process per GPU).  Rank 0 creates the id, the host
 * broadcasts it (torch.distributed), every rank calls fdtd_comm_init.  Faces with
 * FDTD_BC_NEIGHBOR exchange ghost planes with rank-1 / rank+1 (periodic z wraps). */
int fdtd_comm_unique_id(char id[128]);
int fdtd_comm_init(FdtdSolver* h, const char id[128], int rank, int n_ranks);

/* advance n_steps time steps starting at the handle's current step counter: start() + monitor()
 * of the cloud path (ref web/api/webapi.py:266,:337); the step count is Simulation.num_time_steps
 * (ref simulation.py:4226). */
int fdtd_run(FdtdSolver* h, int64_t n_steps, FdtdProgressFn progress, void* user);
/* Bloch boundaries (ref boundary.py:55-79 BlochBoundary: F(r + L_a) = bloch_phase_a F(r), complex
 * fields): two handles created from the same configuration carry the real and the imaginary part
 * (the host gives the second one the source weights times -i) and are advanced together;
 * phase[a] = 2 pi bloch_vec of axis a.  A Bloch axis x or y is laid out by the host with one ghost cell
 * at each end (device index 0 and n_real[a] + 1, PEC faces in FdtdConfig; n_real[a] = 0: no ghost
 * cells on that axis); a Bloch z uses the ghost planes of FDTD_BC_PERIODIC z faces.  On a z-slab
 * (FDTD_BC_NEIGHBOR faces) the first handle carries the communicator (fdtd_comm_init) and both parts
 * exchange their ghost planes through it; planes that wrap around a Bloch z axis are rotated where they
 * arrive.  Fully anisotropic lists (fdtd_add_aniso_bloch) are coupled across the Bloch faces with their phases; not on
 * z-slabs.  Monitors of the pair are read per handle; a value is re + i im. */
int fdtd_run_bloch(FdtdSolver* h_re, FdtdSolver* h_im, int64_t n_steps, const double phase[3], const int n_real[3],
                   FdtdProgressFn progress, void* user);
/* ref web/api/webapi.py:370 (task status incl. "diverged"), web/core/task_core.py:537 (run info) */
int fdtd_get_stats(FdtdSolver* h, FdtdStats* out);
/* tuning knobs that may change between runs of one handle (bench A/B without re-upload).  Each key's comment ends with what the
 * tests establish for it.  "Switched between runs: lifecycle tests" = tests/test_emu_lifecycle.py / tests/test_gpu_lifecycle.py switch
 * it A / B / A inside one engine; the engine ends on the bits of a fresh handle that took single steps, and its per-run counters show
 * the path change and change back.  fdtd_add_point_source, fdtd_add_tfsf and fdtd_add_monitor are accepted between runs as well (a
 * monitor's first record step lies behind the steps done): node tables and paged source tables are rebuilt for the lists of the next
 * run.  fdtd_add_ade is refused once the memory terms are paged. */
enum { FDTD_OPT_FLAGS = 0 /* Not switched between runs by any test. */, FDTD_OPT_VARIANT = 1 /* Switched between runs: lifecycle tests. */, FDTD_OPT_ZCHUNK = 2 /* Switched between runs: lifecycle tests. */, FDTD_OPT_ROWS = 3 /* Switched between runs: lifecycle tests. */, FDTD_OPT_XCD_REMAP = 4 /* tile order of the sweep: -1 = default (runs of 8 tiles per XCD), 0 = plain, 1 = a contiguous eighth per XCD, G > 1 = runs of G tiles. Switched between runs: lifecycle tests. */,
       FDTD_OPT_FUSED_LB = 5 /* Not switched between runs by any test. */,
       FDTD_OPT_PML_FUSED = 6 /* axes (bit mask) whose CPML recursions run inside the fused sweep: -1 = default (one GPU: all; z-slab ranks: slab kernels), 0 = slab kernels, 6 / 7 = y z / all inside the sweep — on z-slab ranks too (set it on every rank). Switched between runs: lifecycle tests. */,
       FDTD_OPT_BND_PLANES = 7 /* planes per boundary chunk of the fused z-slab schedule, 0 = default (2). Not switched between runs by any test. */,
       FDTD_OPT_AUTOTUNE = 8 /* 1: time a few tile shapes of the fused sweep on the first run of grids >= 2^20 cells (default 0). Not switched between runs by any test. */,
       FDTD_OPT_PML_SPLIT = 9 /* CPML-carrying step as three launches over interior / edge tiles: -1 = by grid size (default), 0, 1. Switched between runs: lifecycle tests. */,
       FDTD_OPT_PLACEMENT_TRIES = 12, /* alternative placements of the field arrays the first large one-GPU run samples (0 ... 8, default 6; 0 = keep the first allocations): each costs six sweeps and a further copy of the field memory until the probe ends (candidates that lose are held so that the next one lands elsewhere). Not switched between runs by any test. */
       FDTD_OPT_MEM_HINTS = 11, /* 1 (default): the measured store placement of the sweep (without CPML: non-temporal field stores, H ahead of the row exchange; with CPML: the H-side psi behind the E update); 0: plain stores, fields at the end of the plane, H-side psi in the H phase. Switched between runs: lifecycle tests. */
       FDTD_OPT_TBLOCK = 13, /* one-GPU fused runs without CPML / TFSF / periodic z: advance TWO time steps per pass over
                                the grid, slab by slab (slab s+1 takes step n, then slab s takes step n+1 while the
                                intermediate planes are still in the 256 MiB Infinity Cache): planes per slab; 0 = off,
                                -1 = default. Switched between runs: lifecycle tests. */
       FDTD_OPT_EDGE_ZCHUNK = 14, /* planes per workgroup of the EDGE launches of a CPML step (tiles that meet a y / z slab):
                                     -1 = default (z-slab ranks, where they share the interior launch's stream: about one wave of
                                     workgroups, at least 2 planes; one GPU: as the interior launch), 0 = as the interior launch, N. Switched between runs: lifecycle tests. */
       FDTD_OPT_GRAPH = 15, /* one-GPU fused runs on one stream: steps without monitor records / decay checks replayed as captured
                               hipGraphs of two steps: -1 = default (off: on ROCm 7.2 replaying costs ~3 us per step MORE than the
                               launches it replaces, profiles/r3i), 0 = never, 1 = whenever possible. Switched between runs: lifecycle tests (device; captured graphs live for one fdtd_run, so a change of tile shape or of the source lists between runs cannot meet a stale one). */
       FDTD_OPT_TWOSTEP = 16, /* two time steps per sweep (in-kernel temporal blocking, bit-identical to single steps; non-dispersive media, PEC
                                 walls (PMC allowed on the min faces), absorber layers, point sources while they inject (any sources once
                                 they are spent), small time monitors, DFT monitors, no decay check on the middle step; CPML and periodic
                                 faces through shell pairs (FDTD_OPT_SHELL_PAIRS), z-slab ranks without CPML with their boundary planes as
                                 the shell — everything else takes single steps, FdtdStats.fused2_off_reason says why): -1 = default (on,
                                 tile shape by grid size), 0 = off, else waves per workgroup (4 ... 16; W - 3 rows of a tile are written)
                                 + 64 * planes per chunk (0 = by grid size). Switched between runs (any shape, 0, -1): lifecycle tests. */
       FDTD_OPT_SHELL_PAIRS = 17, /* step pairs on grids with CPML or periodic faces (the two-step sweep over the bulk; the shell — CPML slabs +
                                     a two-cell collar, the two rows / planes next to a periodic y / z face — as two single steps beside it
                                     on the second stream, through a third field set; periodic x wraps inside the sweep; bit-identical to
                                     single steps), and on z-slab ranks: -1 = default (on), 0 = off, 2 = shell behind the bulk on ONE stream
                                     (a measuring aid). Switched between runs: lifecycle tests. */
       FDTD_OPT_STRIP = 18, /* x strips of a shell step: planes per workgroup (1 ... 63) + 64 * workgroups per CU their registers are cut for (3 or 4). Switched between runs: lifecycle tests. */
       FDTD_OPT_SHELL2 = 19, /* the shell of a CPML-walled grid (no periodic z, no absorber layers; a periodic x wraps through the boxes' halo
                                lanes, the rows next to a periodic y wrap and the planes of dispersive cells take single steps beside the
                                boxes; sources that inject three or more cells inside the bulk, or on planes that become z holes; z-slab ranks
                                that carry CPML inside their sweeps too) by shell2_step_kernel — two steps per sweep with psi carried, both
                                psi sides ping-ponged, no third field set; bit-identical to single steps: -1 = default (where the cost
                                model likes it), 0 = off (two single steps beside the bulk, FDTD_OPT_SHELL_PAIRS), 1 = wherever possible, 2 / 3 = wherever possible with
                                one launch per instantiation (x / y / z only, all axes) / per box (measuring aids). Switched between runs: lifecycle tests. */
       FDTD_OPT_SHELL2_SHAPE = 20, /* tile shapes of its launches (one per instantiation: x / y / z only, all axes; each over all of its boxes): lanes
                                      per row of the wide boxes (z / y slabs; 3 ... 64, 0 = by box: the shape that wastes the fewest lane-planes)
                                      + 128 * waves per workgroup of the all-axes launch (1 ... 8, default 8) + 1024 * planes per chunk of the wide
                                      boxes (0 = by box) + 2^17 * waves per workgroup of the one-axis launches (1 ... 8, default 6) + 2^21 * planes
                                      per chunk of the x strips (0 = by box); <= 0: defaults. Switched between runs: lifecycle tests. */
       FDTD_OPT_DEBUG_SYNC = 21, /* 1: a device-wide synchronisation in front of and behind every launch group of fdtd_run (no two launches ever
                                    overlap): a debugging aid — a schedule whose result then differs from the normal run's has a missing
                                    cross-stream edge.  Default 0. A debugging aid; switched between runs: lifecycle tests. */
       FDTD_OPT_TILE_SPLIT = 22, /* the two-step sweep of a grid with bodies: workgroups whose tile (halo rows and planes included) holds only
                                    the background medium run the plain sweep inside the materials launch; same bits: -1 = default (where at
                                    least one tile in eight is background-only), 0 = never, 1 = wherever such a tile exists. Switched between runs: lifecycle tests. */
       FDTD_OPT_DISP = 23, /* dispersive (pole-residue ADE) cells advanced INSIDE the two-step sweeps: their pole states move into paged storage
                              (one block per 256-cell row segment that holds a dispersive cell, two sets) before the first run that may take
                              step pairs, and single steps update them there too.  -1 / 1 = default (on one GPU, where the packed medium words
                              name the ADE group of every dispersive cell), 0 = off: the planes of dispersive cells are z holes of the bulk
                              (single steps, round 5).  Set it before the first fdtd_run. The setter refuses 0 once the memory terms are paged; the handle is unchanged and goes on: lifecycle tests. */
       FDTD_OPT_SRC_PAGED = 25, /* step pairs WHILE a TFSF box, a mode plane, a current sheet or any list of more than 256 nodes injects (round 6):
                                   in front of each pair list kernels leave what the lists add at steps n (E side), n + 1 (H side) and n + 1
                                   (E side) in paged storage — one block per 256-cell row segment that holds a source node — and the
                                   two-step sweep, its seam kernel and the shell's boxes add them.  -1 / 1 = default (on one GPU, where no
                                   two lists meet on a node), 0 = off: single steps (or the lists' planes as z holes) while they inject.  May change
                                   between runs. 0 is honoured on a handle whose tables exist (they are kept and used again when it is switched back).  Switched between runs: lifecycle tests. */
       FDTD_OPT_WHATIF = 24, /* measuring aid (round 6): 1 ... 8 = a what-if instantiation of the vacuum two-step sweep that skips part of its work
                                (csrc/fdtd_kernels2.hpp lists them) — WRONG results, meaningful times; 0 = off (default);
                                16 ... 18 = plain pairs without the seam_kernel launch / with it skipped and the sweep reading the repair array /
                                with seam_kernel storing into the repair array (what deferred seam repair can gain, pays and costs);
                                19 = the vacuum sweep without its one-lane stores into the seam scratch (and without EXJ: compare with 14). A measuring aid; not switched between runs by any test. */
       FDTD_OPT_SLAB_BOXES_FIRST = 26, /* z-slab ranks that carry CPML, step pairs: the shell's boxes are launched in front of the bulk sweep (1), behind it (0: round 5), beside it on a third stream (2), or 2 for slabs of 96 planes and more, else 1 (3, default). Not switched between runs by any test. */
       FDTD_OPT_SEAM_DEFER = 27, /* deferred seam repair: a plain step pair (whole grid, sixteen-wave plain / materials / absorber sweep) that is
                                    followed in the same fdtd_run by another plain pair — no record, decay check, H-side source launch or ghost-plane
                                    copy between them — leaves the seven values seam_kernel repairs per seam row in a compact array the next
                                    sweep's edge lanes read, instead of storing them into the fields at a row stride.  -1 / 1 = on (default):
                                    launches of sixteen-wave workgroups, which run the instantiation that reads the array anyway; 0 = off;
                                    2 = testing aid: at every workgroup size (smaller workgroups then run the sixteen-wave instantiation —
                                    another launch bound than their own, not a setting for production runs).  May be switched between runs of one engine (A/B inside one placement of the arrays). (tests/test_emu_seam_defer.py switches it.) */
       FDTD_OPT_AXIS_SHIFT = 28, /* 0 (default), 1, 2: the caller laid the problem out with its axes cyclically renamed — device axis a holds the
                                    caller's axis (a + s) % 3.  The solve does not depend on it; what is formed axis after axis in a fixed order
                                    does: the passes of a sparse field-time monitor's gather (fdtd_add_field_time_monitor), of a sparse DFT
                                    monitor's colocation (fdtd_add_field_dft_monitor) and of a lattice DFT monitor's sums (fdtd_add_lattice_dft_monitor) then run along the caller's x, y, z, so that the renamed problem gives the bits of the plain one. (tests/test_emu_field_time.py runs all three.) */
       FDTD_OPT_LDS_PAD = 10 /* measuring aid: extra dynamic LDS per workgroup of the sweep in bytes (lowers its occupancy). Not switched between runs by any test. */ };
int fdtd_set_option(FdtdSolver* h, int key, int value);
int fdtd_get_seam_stats(FdtdSolver* h, FdtdSeamStats* out);
int fdtd_reset(FdtdSolver* h);      /* zero fields, auxiliaries, monitors and the step counter */

/* Checkpoint and resume: everything of a handle that evolves from step to step, as one host blob, and back into a fresh handle that
 * was set up the same way (docs/history/CHECKPOINT.md).  The library keeps ONE table of state sections (a device pointer and a byte
 * count each; fdtd_capi.hip state_sections) that fdtd_reset zeroes, fdtd_get_state copies out and fdtd_set_state copies in:
 *   saved    the six live field arrays (ghost planes included), the live CPML psi sets of every axis (E side, H side), e_old and q of
 *            every ADE group, e1 / h1 of every TFSF box, `data` of every monitor and the reduced series / gathered array of a ring
 *            monitor — in this order;
 *   scratch  the other two field sets and the other psi sets: the write sides of the ping-pongs, overwritten before they are read.
 *            Not in the blob; fdtd_set_state zeroes those the handle holds;
 *   derived  the paged ADE memory terms: cc S(Q), a function of q alone.  Not in the blob: they are written in their UNPAGED form (q),
 *            and rebuilt from it by the set-up kernel that laid them out — by fdtd_set_state on a handle that has paged, by the first
 *            fdtd_run on one that has not run yet.
 * Live buffers: the library swaps the POINTERS of its field and psi sets after every sweep, so the arrays a handle calls current are the
 * live ones whatever the step's parity; the blob holds them under that name — a canonical buffer, no index stored — and
 * fdtd_set_state writes them into whatever the receiving handle calls current.
 * Blob = FdtdStateHeader, uint64 section_bytes[n_sections], uint64 {next, reduced}[n_monitors], then the saved sections back to back.
 * The fingerprint hashes what fixes the layout and meaning of the sections: the padded grid and field_bytes; per axis the CPML layer
 * counts and psi entries; comp, n, n_poles of every ADE group; n_aux of every TFSF box; kind, form, data_bytes, result_bytes of every
 * monitor; the counts of anisotropic / modulation / conformal / nonlinear lists.  It does not change with the steps taken or fdtd_reset.
 * fdtd_get_state first synchronises the handle's streams, flushes deferred seam columns and drains the monitor rings, as fdtd_run does
 * on its way out.  fdtd_set_state checks everything before it touches the handle and refuses by name: "bad magic", "format version",
 * "fingerprint", "section ... bytes", "too small".  Handles with a communicator (z-slab ranks) refuse fingerprint, get and set:
 * "state save / restore is not available on z-slab handles".  The two handles of an fdtd_run_bloch pair each have their own blob. */
#define FDTD_STATE_MAGIC "FDTDSTA1"
#define FDTD_STATE_VERSION 1
typedef struct FdtdStateHeader {
  char     magic[8];         /* FDTD_STATE_MAGIC                                             */
  uint64_t version;          /* FDTD_STATE_VERSION                                           */
  uint64_t fingerprint;      /* fdtd_state_fingerprint of the handle that wrote it           */
  int64_t  step;             /* the handle's step counter                                    */
  uint64_t n_sections;
  uint64_t n_monitors;
  double   energy_max;
  int64_t  steps_done;       /* FdtdStats: the four fields fdtd_reset clears                 */
  int64_t  diverged;
  int64_t  stopped_early;
  double   field_decay;
  uint64_t total_bytes;      /* of the whole blob = fdtd_state_bytes                         */
} FdtdStateHeader;
int     fdtd_state_fingerprint(FdtdSolver* h, uint64_t* out);
int64_t fdtd_state_bytes(FdtdSolver* h);                               /* < 0: error */
int     fdtd_get_state(FdtdSolver* h, void* host, size_t bytes);       /* bytes >= fdtd_state_bytes */
int     fdtd_set_state(FdtdSolver* h, const void* host, size_t bytes);

/* Which instantiations of the two-step sweep ran.  fused2_step_kernel<LB, OPT> exists once per listed (LB, OPT) pair (launch bound in
 * threads: 512 / 768 / 1024; OPT: the feature word of tidy3d_amd/csrc/fdtd_fused2.hpp — 1 non-temporal stores, 2 materials, 4 monitor
 * table, 8 absorber layers, 16 clipped to the bulk of a shell pair, 32 dispersive cells, 64 paged source terms, bits 8 - 11 a what-if
 * variant, 8192 deferred seam repair), and a launch runs exactly one of them with W waves (rows) per workgroup.  One int64 per entry:
 * bits 0 - 31 OPT, bits 32 - 47 LB, bits 48 - 55 W. */
#define FDTD_SWEEP_WORD(lb, opt, w) (((int64_t)(w) << 48) | ((int64_t)(lb) << 32) | (int64_t)(opt))
#define FDTD_SWEEP_WORD_OPT(word) ((int)((word) & 0xffffffff))
#define FDTD_SWEEP_WORD_LB(word) ((int)(((word) >> 32) & 0xffff))
#define FDTD_SWEEP_WORD_W(word) ((int)(((word) >> 48) & 0xff))
/* The distinct (LB, OPT, W) this handle has launched since fdtd_create or the last fdtd_reset, in the order of their first launch: returns
 * their number (negative: error) and fills min(number, cap) entries of `out`.  Host bookkeeping only; like FdtdSeamStats, outside FdtdStats. */
int fdtd_get_sweep_words(FdtdSolver* h, int64_t* out, int cap);
/* Every instantiation the library holds, with W = 0: returns their number and fills min(number, cap) entries.  Needs no handle and no device. */
int fdtd_sweep_table(int64_t* out, int cap);

/* Staircase rasterisation of Box, Sphere and Cylinder structures on the device (ref simulation.py:1135-1241; the host form is
 * tidy3d_amd/discretize.py rasterize, which the result equals bit for bit; csrc/fdtd_raster.hpp).  Needs no handle.
 * The job: the grid shape; for each E component c its Yee coordinates along x, y, z (coords[3 c + a]: nx / ny / nz doubles); n records
 * in the order of the structures.  A record paints, per component c, the nodes of the index box [lo[c], hi[c]) (x, y, z; an empty box
 * paints nothing) that pass the primitive's inside test with medium[c]:
 *   FDTD_RASTER_BOX       |p_a - center[a]| <= 0.5 size[a] on every axis a (size[a] may be inf)
 *   FDTD_RASTER_SPHERE    (dx^2 + dy^2) + dz^2 <= size[0]                      size[0] = the squared radius as the caller evaluates it
 *   FDTD_RASTER_CYLINDER  size[0] > 0, d0^2 + d1^2 <= size[0]^2 over the two axes other than `axis` (in x, y, z order) and
 *                         |p_axis - center[axis]| <= 0.5 size[1]               size[0] = radius, size[1] = length (inf allowed)
 * each operation in fp64, rounded once, in the order written.  out_host: uint16 [3][nz][ny][nx]; it starts as 1 (the background) and
 * takes the records one after another on one stream — a later record overwrites an earlier one.  Refused with no launch: a null
 * pointer, n == 0, an unknown kind, an index box outside the shape, a medium index that is no uint16, struct_bytes / record_bytes that
 * are not this header's sizes.  Returns 0, or -1 with fdtd_last_error(NULL). */
enum { FDTD_RASTER_BOX = 0, FDTD_RASTER_SPHERE = 1, FDTD_RASTER_CYLINDER = 2 };
typedef struct FdtdRasterRecord {
  int32_t kind;            /* FDTD_RASTER_*                                               */
  int32_t axis;            /* cylinder: 0, 1, 2                                           */
  int32_t medium[3];       /* table index per E component (0 = PEC)                       */
  int32_t lo[3][3];        /* [component][x, y, z]                                        */
  int32_t hi[3][3];
  int32_t reserved;
  double  center[3];
  double  size[3];
} FdtdRasterRecord;
typedef struct FdtdRasterJob {
  int32_t struct_bytes;    /* sizeof(FdtdRasterJob) of the caller                         */
  int32_t record_bytes;    /* sizeof(FdtdRasterRecord) of the caller                      */
  int32_t device;          /* HIP device ordinal                                          */
  int32_t nx, ny, nz;
  int64_t n;               /* records                                                     */
  const double* coords[9];
  const FdtdRasterRecord* records;
} FdtdRasterJob;
int fdtd_rasterize(const FdtdRasterJob* job, uint16_t* out_host);

#ifdef __cplusplus
}
#endif
#endif /* FDTD_HIP_H */
