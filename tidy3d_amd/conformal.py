"""PEC-conformal boundaries (SubpixelSpec.pec = PECConformal): the Dey-Mittra conformal scheme as edge and face fractions, a
changed E raster and one list of cut faces per H component (spec.ConformalSet).  docs/history/PEC_CONFORMAL.md holds the scheme,
the clamp, the refusals and the figures.

  l    per E node (an edge of the primal grid) the fraction of the edge outside PEC; "PEC" is wherever the staircase rule (the last
       structure that holds the point) finds the PEC medium.  The rule is applied at both end nodes and at the midpoint; where two
       of them differ the crossing is bisected to 2^-21 of the edge, each half on its own.
  A    per H node (a face) the free fraction of its area: the polygon through the edge crossings (a straight cut); faces whose
       crossings do not define one polygon (a diagonal pair of free corners, an edge crossed twice) are sampled 16 x 16.
  A_eff = max(A, CLAMP_FACTOR (1 - timestep_reduction)^2 max_k l_k): the local stability bound (Benkler et al., IEEE TAP 54, 1843
       (2006)) — the operator test of tests/test_emu_pec_conformal.py is its judge.
  E raster: an edge is PEC (index 0) iff l == 0 (l < L_MIN counts as 0); an edge whose midpoint lies in PEC but whose l > 0 takes the
       medium found at the middle of its free part; everything else keeps its index.
  Inside CPML / absorber layers the staircase rule stands (no entries for faces with an edge in a layer); no entries for the H
  nodes on a PEC min wall (their four edges are pinned)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import schema as td
from .coeffs import h_coeff, inv_steps
from .exceptions import Tidy3dNotImplementedError
from .spec import BC_PEC, BC_PERIODIC, ConformalSet, SolverSpec

L_MIN = 1e-3              # an edge with less than this fraction outside PEC is a PEC edge
CLAMP_FACTOR = 1.0        # on the local bound (1 - timestep_reduction)^2 max_k l_k; raised only if the operator test finds a violation
AREA_MIN = 1e-4           # what the weights divide by at the least (below the clamp's own floor CLAMP_FACTOR 0.49 L_MIN unless the clamp is off)
BISECTIONS = 20          # per half edge: 2^-21 of the edge
N_SAMPLE = 16             # per axis, faces without a single straight cut


def pec_conformal_of(sim) -> Optional["td.PECConformal"]:
    """the PECConformal of ``sim.subpixel`` if the scheme is on: a SubpixelSpec that names one and a PEC medium in the simulation"""
    sp = sim.subpixel
    if not isinstance(sp, td.SubpixelSpec) or not isinstance(sp.pec, td.PECConformal):
        return None
    if not any(getattr(m, "is_pec", False) for m in sim.mediums):
        return None
    return sp.pec


class _Scene:
    """the staircase rule at arbitrary points: the last structure that holds a point owns it (Medium2D sheets have no volume)"""

    def __init__(self, sim):
        self.structs = [(st.geometry, bool(getattr(st.medium, "is_pec", False)), st.medium) for st in sim.all_structures
                        if not isinstance(st.medium, td.Medium2D)]
        self.background = sim.medium
        self.first = next(n for n, s in enumerate(self.structs) if s[1])

    def pec_at(self, x, y, z) -> np.ndarray:
        shape = np.broadcast_shapes(np.shape(x), np.shape(y), np.shape(z))
        out = np.zeros(shape, bool)
        for geo, pec, _ in self.structs[self.first:]:
            out[np.broadcast_to(geo.inside(x, y, z), shape)] = pec
        return out

    def pec_on_lattice(self, xs, ys, zs) -> np.ndarray:
        """[nz, ny, nx] over the tensor lattice; every structure is tested inside its bounding box only"""
        out = np.zeros((len(zs), len(ys), len(xs)), bool)
        for geo, pec, _ in self.structs[self.first:]:
            (x0, y0, z0), (x1, y1, z1) = geo.bounds
            r = []
            for cc, lo, hi in ((xs, x0, x1), (ys, y0, y1), (zs, z0, z1)):
                r.append((max(int(np.searchsorted(cc, lo, side="left")) - 1, 0), min(int(np.searchsorted(cc, hi, side="right")) + 1, len(cc))))
            if any(a >= b for a, b in r):
                continue
            sub = out[r[2][0]:r[2][1], r[1][0]:r[1][1], r[0][0]:r[0][1]]
            ins = geo.inside(xs[None, None, r[0][0]:r[0][1]], ys[None, r[1][0]:r[1][1], None], zs[r[2][0]:r[2][1], None, None])
            sub[np.broadcast_to(ins, sub.shape)] = pec
        return out

    def medium_at(self, x, y, z) -> List:
        """the medium object that owns every point (flat arrays)"""
        own = np.full(np.shape(x), -1, np.int64)
        for n, (geo, _, _) in enumerate(self.structs):
            own[np.asarray(geo.inside(x, y, z), bool)] = n
        return [self.background if n < 0 else self.structs[n][2] for n in own]


def _layers(sim, spec: SolverSpec) -> List[Tuple[int, int]]:
    """per axis the (low, high) counts of cells inside CPML or absorber layers"""
    out = []
    for a in range(3):
        lo, hi = int(spec.pml[a][0].num_layers), int(spec.pml[a][1].num_layers)
        if spec.absorber is not None:
            lo, hi = max(lo, int(spec.absorber[a][2])), max(hi, int(spec.absorber[a][3]))
        out.append((lo, hi))
    return out


def _take(arr: np.ndarray, axis: int, sl) -> np.ndarray:
    """arr sliced along the physical axis (arrays are [z, y, x])"""
    idx = [slice(None)] * 3
    idx[2 - axis] = sl
    return arr[tuple(idx)]


def edge_fractions(scene: _Scene, spec: SolverSpec, c: int):
    """-> (l, mid_free): the free fraction of every edge of E component c on the lattice extended to the far nodes (N cells along c,
    N + 1 nodes along the other two axes), and for the cut edges the parameter in [0, 1] of the middle of their free part
    (NaN elsewhere)."""
    b = [np.asarray(v, np.float64) for v in spec.boundaries]
    coords = [0.5 * (b[a][1:] + b[a][:-1]) if a == c else b[a] for a in range(3)]
    nodes = scene.pec_on_lattice(b[0], b[1], b[2])
    end0, end1 = _take(nodes, c, slice(0, -1)), _take(nodes, c, slice(1, None))
    mid = scene.pec_on_lattice(*coords)
    l = np.where(mid, 0.0, 1.0)
    where_free = np.full(l.shape, np.nan)
    cut = (end0 != mid) | (end1 != mid)
    kk, jj, ii = np.nonzero(cut)
    if kk.size == 0:
        return l, where_free
    idx = (ii, jj, kk)
    p0 = [b[a][idx[a]] for a in range(3)]
    length = np.diff(b[c])[idx[c]]

    def at(t):
        p = list(p0)
        p[c] = p0[c] + t * length
        return scene.pec_at(p[0], p[1], p[2])

    flags = [end0[cut], mid[cut], end1[cut]]
    starts, stops = [], []
    for h in (0, 1):                                       # each half on its own: [h / 2, (h + 1) / 2]
        fa, fb = flags[h], flags[h + 1]
        lo, hi = np.full(kk.size, 0.5 * h), np.full(kk.size, 0.5 * (h + 1))
        differ = fa != fb
        for _ in range(BISECTIONS):
            tm = 0.5 * (lo + hi)
            same_as_a = at(tm) == fa
            lo = np.where(differ & same_as_a, tm, lo)
            hi = np.where(differ & ~same_as_a, tm, hi)
        tc = 0.5 * (lo + hi)
        s = np.where(differ, np.where(fa, tc, 0.5 * h), 0.5 * h)
        e = np.where(differ, np.where(fa, 0.5 * (h + 1), tc), np.where(fa, 0.5 * h, 0.5 * (h + 1)))
        starts.append(s)
        stops.append(e)
    len0, len1 = stops[0] - starts[0], stops[1] - starts[1]
    joined = (len0 > 0) & (len1 > 0)                       # both halves free at the midpoint: one free part
    centre = np.where(joined, 0.5 * (starts[0] + stops[1]),
                      np.where(len0 >= len1, 0.5 * (starts[0] + stops[0]), 0.5 * (starts[1] + stops[1])))
    l[cut] = np.clip(len0 + len1, 0.0, 1.0)
    where_free[cut] = centre
    return l, where_free


def _face_area(scene: _Scene, spec: SolverSpec, c: int, ijk: np.ndarray, l4: np.ndarray, corners: np.ndarray) -> np.ndarray:
    """free area fraction of the faces ``ijk`` of H component c from their edge fractions l4 [n, 4] (slot order of ConformalSet) and
    the PEC flags of their corners [n, 4] = (00, 10, 01, 11) in (a1, a2)"""
    free = ~corners
    n_free = free.sum(axis=1)
    l_r, l_l, l_t, l_b = l4[:, 0], l4[:, 1], l4[:, 2], l4[:, 3]
    # an edge is "simple" when its fraction is what one crossing between its end flags allows
    ends = {0: (1, 3), 1: (0, 2), 2: (2, 3), 3: (0, 1)}
    simple = np.ones(len(ijk), bool)
    for k, (p, q) in ends.items():
        both_free, both_pec = free[:, p] & free[:, q], corners[:, p] & corners[:, q]
        simple &= np.where(both_free, l4[:, k] == 1.0, np.where(both_pec, l4[:, k] == 0.0, True))
    adj = {0: (l_b, l_l), 1: (l_b, l_r), 2: (l_t, l_l), 3: (l_t, l_r)}          # the two edges that meet at corner p
    area = np.full(len(ijk), np.nan)
    area[simple & (n_free == 4)] = 1.0
    area[simple & (n_free == 0)] = 0.0
    for p, (e1, e2) in adj.items():
        one = simple & (n_free == 1) & free[:, p]
        area[one] = 0.5 * e1[one] * e2[one]
        three = simple & (n_free == 3) & corners[:, p]
        area[three] = 1.0 - 0.5 * (1.0 - e1[three]) * (1.0 - e2[three])
    two = simple & (n_free == 2)
    along_u = two & (corners[:, 0] == corners[:, 1]) & (corners[:, 2] == corners[:, 3])     # the cut crosses the left and right edges
    along_v = two & (corners[:, 0] == corners[:, 2]) & (corners[:, 1] == corners[:, 3])
    area[along_u] = 0.5 * (l_l[along_u] + l_r[along_u])
    area[along_v] = 0.5 * (l_b[along_v] + l_t[along_v])
    rest = np.flatnonzero(np.isnan(area))
    if rest.size:
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        b = [np.asarray(v, np.float64) for v in spec.boundaries]
        t = (np.arange(N_SAMPLE) + 0.5) / N_SAMPLE
        tu, tv = np.meshgrid(t, t, indexing="ij")
        p = [np.repeat(b[a][ijk[rest, a]][:, None], N_SAMPLE * N_SAMPLE, axis=1) for a in range(3)]
        p[a1] = p[a1] + tu.reshape(1, -1) * np.diff(b[a1])[ijk[rest, a1]][:, None]
        p[a2] = p[a2] + tv.reshape(1, -1) * np.diff(b[a2])[ijk[rest, a2]][:, None]
        area[rest] = 1.0 - scene.pec_at(p[0], p[1], p[2]).mean(axis=1)
    return area


def apply_pec_conformal(sim, spec: SolverSpec, clamp: Optional[float] = None) -> None:
    """Changes ``spec.mat_idx`` / ``spec.media`` to the conformal E raster and fills ``spec.conformal``.  ``clamp``: the factor on
    max_k l_k below which the area is not allowed to fall (None: CLAMP_FACTOR (1 - timestep_reduction)^2; 0 switches the clamp
    off — the operator test's counter-example)."""
    from .discretize import MAX_MEDIA, medium_coeffs
    pc = pec_conformal_of(sim)
    if pc is None or spec.mat_idx is None:
        return
    if clamp is None:
        clamp = CLAMP_FACTOR * (1.0 - pc.timestep_reduction) ** 2
    if spec.bloch is not None:
        raise Tidy3dNotImplementedError("PECConformal together with Bloch boundaries is not supported (Staircasing is)")
    if spec.aniso:
        raise Tidy3dNotImplementedError("PECConformal together with FullyAnisotropicMedium is not supported (Staircasing is)")
    if spec.modulation:
        raise Tidy3dNotImplementedError("PECConformal together with time-modulated (modulation_spec) media is not supported (Staircasing is)")
    scene = _Scene(sim)
    shape = spec.shape
    layers = _layers(sim, spec)
    periodic = [spec.bc[a][0] == BC_PERIODIC for a in range(3)]
    mat = spec.mat_idx
    ls = []
    for c in range(3):
        l, where_free = edge_fractions(scene, spec, c)
        # the real edges: N per axis; the far nodes of the other two axes are the wall's edges, or the wrapped ones
        real = tuple(slice(0, shape[a]) for a in (2, 1, 0))
        stair_pec = mat[c] == 0
        cut = ~np.isnan(where_free[real])
        in_layer = np.zeros(stair_pec.shape, bool)
        for a in range(3):
            n_lo, n_hi = layers[a]
            i = np.arange(shape[a])
            shp = [1, 1, 1]
            shp[2 - a] = -1
            in_layer |= ((i < n_lo) | (i >= shape[a] - n_hi)).reshape(shp)
        lr = l[real]
        lr[lr < L_MIN] = 0.0
        keep = in_layer | ~cut                             # the staircase rule stands: inside the layers, and away from the surface
        lr[keep] = np.where(stair_pec[keep], 0.0, 1.0)
        to_pec = ~keep & (lr == 0.0) & ~stair_pec
        mat[c][to_pec] = 0
        to_free = np.nonzero(~keep & (lr > 0.0) & stair_pec)
        if to_free[0].size:
            kk, jj, ii = to_free
            idx = (ii, jj, kk)
            b = [np.asarray(v, np.float64) for v in spec.boundaries]
            p = [b[a][idx[a]] for a in range(3)]
            p[c] = p[c] + where_free[real][to_free] * np.diff(b[c])[idx[c]]
            owners = scene.medium_at(p[0], p[1], p[2])
            new = np.empty(kk.size, mat.dtype)
            cache = {}
            for n, med in enumerate(owners):
                if id(med) not in cache:
                    if getattr(med, "is_pec", False):      # (the bisected point fell back into PEC by a rounding: a PEC edge)
                        cache[id(med)] = 0
                    else:
                        if isinstance(med, (td.AnisotropicMedium, td.FullyAnisotropicMedium)):
                            med = med.component(c)
                        if getattr(med, "is_custom", False) or getattr(med, "is_custom_dispersive", False) or isinstance(med, td.Unsupported):
                            raise Tidy3dNotImplementedError("PECConformal: a spatially varying (Custom*) medium at a PEC surface is "
                                                            "not supported (Staircasing is)")
                        mc = medium_coeffs(med)
                        if mc not in spec.media:
                            if len(spec.media) >= MAX_MEDIA:
                                raise Tidy3dNotImplementedError("more than %d distinct media" % (MAX_MEDIA - 1))
                            spec.media.append(mc)
                        cache[id(med)] = spec.media.index(mc)
                new[n] = cache[id(owners[n])]
            mat[c][to_free] = new
            lr[to_free] = np.where(new == 0, 0.0, lr[to_free])
        l[real] = lr
        for a in range(3):                                 # the far nodes of a periodic axis are the wrapped ones
            if a != c and periodic[a]:
                _take(l, a, slice(-1, None))[...] = _take(l, a, slice(0, 1))
        ls.append(l)
    nodes = scene.pec_on_lattice(*[np.asarray(v, np.float64) for v in spec.boundaries])
    for a in range(3):
        if periodic[a]:
            _take(nodes, a, slice(-1, None))[...] = _take(nodes, a, slice(0, 1))
    ip, _ = inv_steps(spec)
    ch = float(np.float32(h_coeff(spec.dt)))
    spec.conformal = []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        own, up = slice(0, -1), slice(1, None)
        # slot order of ConformalSet: E_a2 up along a1, E_a2 own, E_a1 up along a2, E_a1 own
        e2 = _take(ls[a2], c, own)                         # [N + 1 along a1, N along a2, N along c]
        e1 = _take(ls[a1], c, own)
        l4 = np.stack([_take(e2, a1, up), _take(e2, a1, own), _take(e1, a2, up), _take(e1, a2, own)], axis=-1)     # [nz, ny, nx, 4]
        listed = (l4 != 1.0).any(axis=-1) & (l4 != 0.0).any(axis=-1)
        for a in range(3):                                 # no entries for faces with an edge in a layer
            n_lo, n_hi = layers[a]
            if n_lo + n_hi == 0:
                continue
            i = np.arange(shape[a])
            reach = 1 if a != c else 0                     # the face's edges reach one node up along a1 and a2
            bad = (i < n_lo) | (i + reach >= shape[a] - n_hi)
            shp = [1, 1, 1]
            shp[2 - a] = -1
            listed &= ~bad.reshape(shp)
        if spec.bc[c][0] == BC_PEC:                        # H normal to a PEC min wall, on the wall: its four edges are pinned
            _take(listed, c, slice(0, 1))[...] = False
        kk, jj, ii = np.nonzero(listed)
        if kk.size == 0:
            continue
        ijk = np.stack([ii, jj, kk], axis=1).astype(np.int64)
        lk = l4[kk, jj, ii]
        nc = _take(nodes, c, own)
        corners = np.stack([_take(_take(nc, a1, s1), a2, s2)[kk, jj, ii] for s2 in (own, up) for s1 in (own, up)], axis=1)
        area = _face_area(scene, spec, c, ijk, lk, corners)
        area_eff = np.maximum(np.maximum(area, clamp * lk.max(axis=1)), AREA_MIN)
        nbr = np.repeat(ijk[:, None, :], 4, axis=1)
        nbr[:, 0, a1] += 1
        nbr[:, 2, a2] += 1
        for slot, a in ((0, a1), (2, a2)):
            over = nbr[:, slot, a] >= shape[a]
            if periodic[a]:
                nbr[over, slot, a] = 0
            else:
                nbr[over, slot, :] = -1
        nbr[lk == 0.0] = -1                                # PEC edges: E is zero there
        sign = np.array([1.0, -1.0, -1.0, 1.0])
        inv = np.stack([np.float32(ip[a1])[ijk[:, a1]]] * 2 + [np.float32(ip[a2])[ijk[:, a2]]] * 2, axis=1).astype(np.float64)
        d = -ch * sign[None, :] * (lk / area_eff[:, None] - 1.0) * inv
        d[nbr[:, :, 0] < 0] = 0.0
        spec.conformal.append(ConformalSet(comp=3 + c, ijk=ijk, nbr_comp=(a2, a2, a1, a1), nbr_ijk=nbr, d=d.astype(np.float32),
                                           l=lk.copy(), area=area, area_eff=area_eff))
