"""SolverSpec: the tidy3d-free, plain-array statement of one FDTD run.

This is the stratum between the schema (``tidy3d_amd.schema`` / a real
``tidy3d.Simulation``) and the two consumers that must agree bit-for-bit on
*what* is being solved: the HIP engine (``tidy3d_amd.engine`` ->
``libfdtd_hip.so``) and the fp64 NumPy oracle (``oracle/fdtd_numpy.py``).
Everything here is numpy arrays and POD scalars (SURVEY.md section 7 "Design stance").

Array layout convention (identical on host, in the oracle and in HBM):
fields are ``[nz][ny][nx]`` C-ordered, i.e. **x is the fastest index**; an
xy-plane of one component is one contiguous block (what a z-slab halo
exchange sends).  Yee staggering follows reference grid/grid.py:465-491:
``Ex[k,j,i]`` sits at (xc[i], yb[j], zb[k]), ``Hx[k,j,i]`` at (xb[i], yc[j], zc[k]),
with ``b`` = cell boundaries and ``c`` = cell centres.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from .exceptions import Tidy3dNotImplementedError

COMPONENTS = ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")
COMP_ID = {c: i for i, c in enumerate(COMPONENTS)}

BC_PEC = 0        # tangential E = 0 on the wall (also what backs every PML)
BC_PMC = 1        # tangential H = 0 on the wall (supported on the min side only)
BC_PERIODIC = 2


@dataclass
class MediumCoeffs:
    """One entry of the material table; index 0 is always PEC."""

    eps_inf: float = 1.0
    sigma: float = 0.0                                   # S/um
    poles: Tuple[Tuple[complex, complex], ...] = ()      # (a_k, c_k) rad/s, ref medium.py:2900
    pec: bool = False
    name: str = ""


@dataclass
class AnisoSet:
    """Off-diagonal coupling of one E component inside fully anisotropic bodies (ref medium.py:5058).  The sweep advances
    E_a with the diagonal part, (dt / eps0) [eps^-1]_aa curl_a (a table medium of permittivity 1 / [eps^-1]_aa); this adds

        dE_a(i) = (dt / eps0) sum_{b != a} sum_{j in the four E_b nodes around i} g(i, j) curl_b(j),
        g(i, j) = ([eps^-1]_ab at i + [eps^-1]_ab at j) / 8        (0 outside such bodies)

    — the symmetric average keeps the discrete operator self-adjoint (stable, reciprocal) across body faces; curl_b(j) is
    recovered from what the sweep did to E_b(j): (E_b^{n+1} - Ca E_b^n) / Cb."""

    comp: int                         # a
    ijk: np.ndarray                   # [n, 3] nodes (i, j, k)
    nbr_comp: Tuple[int, ...]         # [8]: slots 0-3 component (a+1)%3, 4-7 component (a+2)%3
    nbr_ijk: np.ndarray               # [n, 8, 3]; -1 = no node (beyond a non-periodic wall)
    g: np.ndarray                     # [n, 8] float64
    nbr_wrap: Optional[np.ndarray] = None   # [n, 8, 3] int8: the period crossed along each axis to reach nbr_ijk (-1, 0, +1;
                                            # periodic axes wrap nbr_ijk into the grid) — a Bloch face multiplies that node by
                                            # exp(i s phi)


@dataclass
class ModulationSet:
    """The nodes of one E component inside one time-modulated medium (ref time_modulation.py ModulationSpec):

        eps(t) = eps_bar + Re[d_eps exp(-2 pi i freq_eps t)],    sigma(t) = sigma_bar + Re[d_sigma exp(-2 pi i freq_sigma t)]

    eps_bar, sigma_bar are the node's own static table medium (``mat_idx``, sub-pixel value included); d_eps, d_sigma carry the
    space modulation at the node's Yee location times the time modulation's amplitude exp(i phase).  The sweep advances the node
    with the static medium, E_lin = Ca E^n + Cb K; the solver replaces that by the update of
    (D^{n+1} - D^n) / dt + sigma^{n+1/2} (E^{n+1} + E^n) / 2 = K, D = eps0 eps(t) E (csrc/fdtd_modulation.hpp)."""

    comp: int                         # E component
    ijk: np.ndarray                   # [n, 3] nodes (i, j, k), each at most once per component
    d_eps: np.ndarray                 # complex128 [n]
    d_sigma: np.ndarray               # complex128 [n], S/um
    freq_eps: float                   # Hz (0 with d_eps = 0: no permittivity modulation)
    freq_sigma: float


@dataclass
class ConformalSet:
    """The faces of one H component cut by a PEC surface under the Dey-Mittra conformal scheme (SubpixelSpec.pec = PECConformal;
    tidy3d_amd/conformal.py, docs/history/PEC_CONFORMAL.md).  A cut face is advanced with

        H_c^{n+1/2} = H_c^{n-1/2} - (dt / mu0) / (A S) sum_k s_k l_k L_k E_k^n,      k = its four edges

    (l_k the free fraction of edge k, A the free fraction of the face's area, enlarged to ``area_eff`` for stability).  The sweep
    applies the same sum with l_k / A = 1, so the solver adds, in front of the sweep,  H_c += sum_k d[k] E_k^n  with
    d[k] = -(dt / mu0) s_k (l_k / area_eff - 1) / step_k (csrc/fdtd_conformal.hpp).  Slots: c = comp - 3, a1 = (c + 1) % 3,
    a2 = (c + 2) % 3;  k = 0: E_a2 one node up along a1 (s = +1), 1: E_a2 at the face's own index (-1), 2: E_a1 one node up along
    a2 (-1), 3: E_a1 at the face's own index (+1); step_k the primal step along a1 (k = 0, 1) or a2 (k = 2, 3)."""

    comp: int                         # H component, 3..5
    ijk: np.ndarray                   # [n, 3] faces (i, j, k), each at most once
    nbr_comp: Tuple[int, ...]         # [4] E component of every slot
    nbr_ijk: np.ndarray               # [n, 4, 3]; -1 = no node (a PEC edge, or beyond a non-periodic wall): E is zero there
    d: np.ndarray                     # [n, 4] float32
    l: np.ndarray                     # [n, 4] float64 free fractions of the four edges
    area: np.ndarray                  # [n] float64 free fraction of the face (a straight cut through the edge crossings)
    area_eff: np.ndarray              # [n] float64 what the weights divide by: max(area, clamp * max_k l_k)


@dataclass
class NonlinearSet:
    """The nodes of one E component inside Kerr media (ref medium.py NonlinearSpec with NonlinearSusceptibility models), merged over
    the media:  D = eps0 (eps_bar + chi3 I) E,  I = E_a^2 + (mean of the four surrounding E_b nodes)^2 + (mean of the four surrounding
    E_c nodes)^2.  eps_bar and the conductivity are the node's own static table medium (``mat_idx``, sub-pixel value included).  The
    sweep advances the node with the static medium, E_lin = Ca E^n + Cb K; the solver replaces that by ``num_iters`` Jacobi
    fixed-point iterations of (D^{n+1} - D^n) / dt + sigma (E^{n+1} + E^n) / 2 = K (csrc/fdtd_nonlinear.hpp)."""

    comp: int                         # E component a
    ijk: np.ndarray                   # [n, 3] nodes (i, j, k), each at most once
    nbr_comp: Tuple[int, ...]         # [8] component of every slot: four of b = (a + 1) % 3, four of c = (a + 2) % 3
    nbr_ijk: np.ndarray               # [n, 8, 3], the layout of AnisoSet.nbr_ijk; -1 = no node (beyond a non-periodic wall): 0 in its mean
    chi3: np.ndarray                  # float64 [n], um^2 / V^2
    num_iters: int = 5                # the same in every set of a spec


# The whole-grid node lists (csrc/fdtd_capi.hip kListKind) by their attribute on the SolverSpec: what the refusals call the kind, its verb
LIST_KINDS = {"aniso": ("FullyAnisotropicMedium", "is"), "modulation": ("time-modulated (modulation_spec) media", "are"),
              "conformal": ("PECConformal", "is"), "nonlinear": ("nonlinear (nonlinear_spec) media", "are")}


def refuse_together(kind, other, hint=""):
    """``kind`` (a key of LIST_KINDS) together with ``other`` (another key, or a phrase) is not supported"""
    phrase, verb = LIST_KINDS[kind]
    raise Tidy3dNotImplementedError(f"{phrase} together with {LIST_KINDS.get(other, (other,))[0]} {verb} not supported{hint}")


@dataclass
class PmlFace:
    """CPML profile of one face (ref boundary.py:195-254; units of sigma/alpha: 2 eps0/dt)."""

    num_layers: int = 0
    sigma_order: int = 3
    sigma_min: float = 0.0
    sigma_max: float = 1.5
    kappa_order: int = 3
    kappa_min: float = 1.0
    kappa_max: float = 3.0
    alpha_order: int = 1
    alpha_min: float = 0.0
    alpha_max: float = 0.0


@dataclass
class PointSourceSet:
    """A current source as a list of Yee points with complex weights and one complex
    waveform:  F[idx] += Re( (w_re + i w_im) * wave[n] ).

    E components (electric current J) are added during the E-update with the waveform
    sampled at t_{n+1/2}; H components (magnetic current M) during the H-update with the
    waveform sampled at t_n.  The weights already contain the update coefficient of the
    cell (-Cb / cell measure for J, -(dt/mu0) / cell measure for M)."""

    comp: np.ndarray            # int32 [n]   component id 0..5
    ijk: np.ndarray             # int32 [n,3] (i, j, k) global Yee indices
    w_re: np.ndarray            # float64 [n]
    w_im: np.ndarray            # float64 [n]
    wave_e: np.ndarray          # complex128 [n_steps]  amp(t_n + dt/2)
    wave_h: np.ndarray          # complex128 [n_steps]  amp(t_n)
    name: str = ""


@dataclass
class TfsfSpec:
    """Axis-aligned total-field/scattered-field source, reduced to plain lists.

    A 1-D auxiliary Yee grid along the propagation axis carries the incident plane wave
    (``e1`` on the n_aux+1 cell boundaries, ``h1`` on the n_aux centres; same steps and dt
    as the 3-D grid, so its numerical dispersion matches the 3-D grid's exactly for
    axis-aligned propagation).  Per step:

      H-phase:  H[comp][ijk] += h_corr_w * e1[h_corr_aux]       (e1 at t_n)
                h1 = ah * h1 - bh * (e1[1:] - e1[:-1])
      E-phase:  E[comp][ijk] += e_corr_w * h1[e_corr_aux]       (h1 at t_n + dt/2)
                e1[1:-1] = ae[1:-1] * e1[1:-1] - be[1:-1] * (h1[1:] - h1[:-1]);  e1[0] = e1[-1] = 0
                e1[src_cell] += wave[n]

    The 1-D grid extends beyond the 3-D domain and ends in matched lossy pads (graded electric
    and magnetic conductivity, reflection-free in 1-D), which is what the per-node decay / update
    coefficients ae, be, ah, bh encode.

    The correction lists (built on the host by ``tidy3d_amd.discretize``) hold every 3-D
    node whose curl stencil straddles the TFSF surface, with the signed update coefficient
    of that node folded into the weight."""

    n_aux: int
    ae: np.ndarray              # float64 [n_aux+1]  decay of e1
    be: np.ndarray              # float64 [n_aux+1]  update coefficient of e1 (sign included)
    ah: np.ndarray              # float64 [n_aux]    decay of h1
    bh: np.ndarray              # float64 [n_aux]    update coefficient of h1 (sign included)
    src_cell: int
    wave: np.ndarray            # float64 [n_steps]
    e_corr_comp: np.ndarray     # int32 [ne]
    e_corr_ijk: np.ndarray      # int32 [ne, 3]
    e_corr_w: np.ndarray        # float64 [ne]
    e_corr_aux: np.ndarray      # int32 [ne]
    h_corr_comp: np.ndarray     # int32 [nh]  (3..5)
    h_corr_ijk: np.ndarray      # int32 [nh, 3]
    h_corr_w: np.ndarray        # float64 [nh]
    h_corr_aux: np.ndarray      # int32 [nh]
    name: str = ""


# MonitorSpec kinds whose result holds the kept nodes only, interpolated on the device by per-component ``taps``
SPARSE_KINDS = ("time_sparse", "dft_sparse", "dft_lattice")


@dataclass
class MonitorSpec:
    """A recorder over a raw Yee index box [lo, hi) (same box for every component).

    kind "time": every recorded step stores the raw component values (H averaged to t_n).
    kind "dft" : running DFT  acc[f] += field * phase[n, f];  E uses phase_e (time t_n),
                 H uses phase_h (time t_n + dt/2).  ``steps`` lists the time-step indices
                 on which the monitor records.
    kind "flux_time": the flux through one planar surface at every recorded step, reduced on the device (float32 [n_rec];
                 csrc/fdtd_flux_time.hpp): flux = sign * sum over the primal nodes of the surface of (E x H) . n_axis times the
                 node's integration weight, each component colocated to the node from the raw box [lo, hi) by ``taps``.
                 ``comps`` = (E_t1, E_t2, H_t1, H_t2) with t1, t2 = axis + 1, axis + 2 (cyclic).
    kind "time_sparse": a time monitor whose result holds only the nodes the user keeps, gathered on the device
                 (csrc/fdtd_field_time.hpp): float32 [n_rec, sum over ``comps`` of the component's kept nodes], inside a record the
                 components one after the other, each [nz_t][ny_t][nx_t].  Every value is the separable linear interpolation ``taps``
                 describe from the raw box [lo, hi): the colocated, downsampled primal nodes (colocate=True) or the downsampled Yee
                 nodes of the component (colocate=False; the node counts then differ between components).
    kind "dft_sparse": a running DFT accumulated on the nodes the user keeps only (csrc/fdtd_field_dft.hpp): complex64 [nf, sum over
                 ``comps`` of the component's kept nodes], inside a frequency the components one after the other, each
                 [nz_t][ny_t][nx_t].  Recorded like kind "dft" (``freqs``, ``phase_e``, ``phase_h``); every sample is interpolated onto
                 the kept nodes by ``taps`` (as kind "time_sparse") before it is accumulated.
    kind "dft_lattice": one surface of a projection monitor accumulated on its sampling lattice only (csrc/fdtd_lattice_dft.hpp):
                 everything as kind "dft_sparse", but ``taps`` carry four taps per node and axis (``data.lattice_taps``: colocation to
                 the primal nodes followed by the resampling to the lattice) and the kept nodes are the lattice points."""

    kind: str
    comps: Tuple[int, ...]
    lo: Tuple[int, int, int]
    hi: Tuple[int, int, int]
    steps: np.ndarray                                   # int64 [n_rec]
    freqs: Optional[np.ndarray] = None                  # float64 [nf]          (dft)
    phase_e: Optional[np.ndarray] = None                # complex128 [n_rec,nf] (dft)
    phase_h: Optional[np.ndarray] = None                # complex128 [n_rec,nf] (dft)
    name: str = ""
    # how the phase tables were formed (the oracle re-derives them from these): recording stride in steps
    # and the apodisation window (start, end, width) or None
    stride: Optional[int] = None
    apod: Optional[Tuple[Optional[float], Optional[float], Optional[float]]] = None
    # kind "flux_time"
    axis: Optional[int] = None                          # normal of the surface
    sign: float = 1.0                                   # its orientation
    taps: Optional[Tuple] = None                        # per axis (index int32 [4, n_t, 2], weight float64 [4, n_t, 2]) into the box, components as ``comps``
    #                                                     kinds "time_sparse", "dft_sparse": per component of ``comps``, per axis (index int32 [n_t, 2], weight float64 [n_t, 2])
    #                                                     kind "dft_lattice": likewise, [n_t, 4]
    weights: Optional[Tuple] = None                     # per axis float64 [n_t] integration weights ([1.] along the normal)
    staging_bytes: int = 0                              # device staging budget (0: the library's default)

    @property
    def targets(self) -> Tuple[Tuple[int, int, int], ...]:
        """kinds "time_sparse", "dft_sparse", "dft_lattice": (nx_t, ny_t, nz_t) kept nodes of every component."""
        return tuple(tuple(int(len(t[a][0])) for a in range(3)) for t in self.taps)

    @property
    def shape(self) -> Tuple[int, int, int]:
        """(bz, by, bx) extents of the recorded box."""
        return (self.hi[2] - self.lo[2], self.hi[1] - self.lo[1], self.hi[0] - self.lo[0])


@dataclass
class SolverSpec:
    shape: Tuple[int, int, int]                         # (nx, ny, nz) cells incl. PML cells
    boundaries: Tuple[np.ndarray, np.ndarray, np.ndarray]   # cell boundaries, N+1 each
    dt: float
    n_steps: int
    bc: Tuple[Tuple[int, int], ...] = ((0, 0), (0, 0), (0, 0))   # [axis][minus, plus]
    pml: Tuple[Tuple[PmlFace, PmlFace], ...] = None
    media: List[MediumCoeffs] = field(default_factory=list)      # [0] = PEC, [1] = background
    mat_idx: Optional[np.ndarray] = None                # uint16 [3, nz, ny, nx] (< 1024); None = all [1]
    sources: List[PointSourceSet] = field(default_factory=list)
    tfsf: List[TfsfSpec] = field(default_factory=list)
    monitors: List[MonitorSpec] = field(default_factory=list)
    # Absorber layers (ref boundary.py:427): per axis (sigma at cell boundaries [N], sigma at cell
    # centres [N], n_lo, n_hi), sigma in units of 2 eps0/dt; None = no absorber (coeffs.damping_tables)
    absorber: Optional[List[Tuple[np.ndarray, np.ndarray, int, int]]] = None
    # Bloch boundaries (ref boundary.py:55-79): phase advance 2 pi bloch_vec per axis across the domain,
    # F(r + L_a) = exp(i bloch[a]) F(r), on axes whose bc is BC_PERIODIC; None = real fields
    bloch: Optional[Tuple[float, float, float]] = None
    # PMC on PLUS faces (ref boundary.py:45 PMCBoundary on any face): per axis the index N of the wall (a cell boundary), or
    # -1.  The grid then carries two ghost cells beyond the wall (shape[a] == N + 2): the wall nodes themselves (tangential
    # E, normal H at index N) are unknowns, everything beyond is the mirror image of the inside — E_tan, H_norm even,
    # E_norm, H_tan odd — refreshed at the start of every step (discretize._discretize_pmc_plus, kernel mirror_fill_kernel)
    mirror_plus: Optional[Tuple[int, int, int]] = None
    aniso: List[AnisoSet] = field(default_factory=list)   # fully anisotropic bodies: off-diagonal coupling per E component
    modulation: List[ModulationSet] = field(default_factory=list)   # time-modulated media: their nodes per E component and medium
    conformal: List[ConformalSet] = field(default_factory=list)     # PEC-conformal boundaries: the cut faces per H component
    nonlinear: List[NonlinearSet] = field(default_factory=list)     # Kerr media: their nodes, one set per E component
    shutoff: float = 0.0                                # 0 disables the early stop
    decay_every: int = 0                                # 0 = never evaluate field decay
    decay_ref_step: int = 0                             # steps before this never shut off
    raster_log: str = ""                                # what discretize.rasterize did, as SimulationData.log words it

    def __post_init__(self):
        if self.pml is None:
            self.pml = tuple((PmlFace(), PmlFace()) for _ in range(3))
        if not self.media:
            self.media = [MediumCoeffs(pec=True, name="PEC"), MediumCoeffs(name="vacuum")]

    # ---- derived 1-D geometry ------------------------------------------------------
    @property
    def n_cells(self) -> int:
        nx, ny, nz = self.shape
        return nx * ny * nz

    def primal_steps(self, axis: int) -> np.ndarray:
        """d[i] = b[i+1] - b[i]   (ref grid.py:393-401)."""
        return np.diff(np.asarray(self.boundaries[axis], dtype=np.float64))

    def dual_steps(self, axis: int) -> np.ndarray:
        """dd[i] = (d[i] + d[i-1]) / 2; d[-1] wraps for periodic axes and mirrors (= d[0])
        otherwise (ref grid.py:404-417 uses the periodic roll; the mirror value is only ever
        used by the PMC rule since PEC zeroes the wall component)."""
        d = self.primal_steps(axis)
        prev = np.roll(d, 1)
        if self.bc[axis][0] != BC_PERIODIC:
            prev[0] = d[0]
        return 0.5 * (d + prev)

    def centers(self, axis: int) -> np.ndarray:
        b = np.asarray(self.boundaries[axis], dtype=np.float64)
        return 0.5 * (b[1:] + b[:-1])

    def yee_coords(self, comp: int):
        """(x, y, z) 1-D coordinate arrays (length N each) of component ``comp``
        (ref grid.py:465-491)."""
        is_h = comp >= 3
        a = comp % 3
        out = []
        for ax in range(3):
            b = np.asarray(self.boundaries[ax], dtype=np.float64)
            on_center = (ax == a) != is_h      # E: centre along own axis; H: centre along others
            out.append(0.5 * (b[1:] + b[:-1]) if on_center else b[:-1])
        return tuple(out)
