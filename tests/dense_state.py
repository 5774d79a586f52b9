"""Dense random states held to the fp64 oracle node by node: the helper shared by tests/test_emu_dense_state.py (emulator) and
tests/test_gpu_dense_state.py (device).  docs/history/DENSE_STATE.md holds the figures.

The other oracle comparisons drive a few dipoles for 60 - 100 steps and take one whole-array rel-L2 figure per component: a
coefficient wrong at one node, or in a plane where little field arrives, weighs nothing in it.  Here every node carries field from
step 0 on and every node is judged against what stands around IT:

  state    six fields, a seeded sum of twelve plane waves of random direction (wavelength 6 - 16 cells, in index space, so that graded
           axes are filled alike) plus 10 % white noise; E of amplitude 1e-3, H of 1e-3 / eta0; complex under Bloch phases; rounded to
           fp32 before either side sees it.  Nodes the scheme pins (tangential E on PEC walls, PEC bodies) are found from the ORACLE
           — one fp64 step from an all-non-zero state, the nodes left at exactly 0 — and set to zero; what lies beyond a PMC-plus wall
           is zero too and cropped as ``cases.run_case`` crops it.  Nothing else is excluded.
  measure  per component, |got - ref| / scale at every node, H times eta0; scale = the largest |ref| over the node's 3 x 3 x 3
           neighbourhood and the six components at the first and the last step, floored at 1e-3 of the global rms: computed from
           the fp64 reference alone.  The worst node per component comes with its index and what lies there.  Monitor records
           likewise, element by element, against the record's own neighbourhood.
  floor    the same measure between OracleFdtd(spec, dtype=np.float32) and the fp64 oracle from the same state.
  bar      MARGIN x floor of the case and K."""
import dataclasses

import numpy as np

from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.spec import BC_PERIODIC

from cases import CASES

ETA0 = 376.730313668
AMP = 1e-3
N_WAVES = 12
NOISE = 0.1
SCALE_FLOOR = 1e-3            # x the global rms
# One margin for every case, K and path.  The fp32 oracle rounds every stored value ONCE per update (its arithmetic between two
# stores runs in fp64: the coefficient tables stay float64 and promote every product); a kernel rounds every operation of the same
# update in fp32 — two differences, their 1/step products, the CPML pair (kinv d + psi) per difference, the Ca / Cb (or dt/mu0)
# products, FMA-contracted and associated in another order: four to eight roundings of terms that are each as large as the result
# (Courant number ~ 0.57 per difference) where the oracle has one.  Errors of K steps add in both alike.  Hence a small integer
# multiple of the floor: 8.
MARGIN = 8.0
KS = (1, 2, 6)
COMP = ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")
PATHS = ("fused", "twopass", "pairs")
X_TILE = 256                  # cells per x tile of the sweeps: seams at its multiples


# ---------------------------------------------------------------------------------------------------------------- specs
def case_spec(name, shape=None, n_steps=max(KS), **kw):
    """SolverSpec of ``cases.CASES[name]`` at its default shape, or at ``shape`` (cells; au_array keeps its cell count per
    feature: the step shrinks with the first axis as tests/test_gpu_shell_pairs.py has it)."""
    fn = CASES[name]
    if shape is None:
        sim = fn(**kw)
    elif name == "au_array":
        sim = fn(tuple(shape), fn.__defaults__[1] * fn.__defaults__[0][0] / shape[0])
    else:
        sim = fn(tuple(shape), **kw)
    spec = discretize(sim, n_steps=n_steps).spec
    spec.decay_every = 0
    return spec


def times(name, k=3):
    return tuple(int(n * k) for n in CASES[name].__defaults__[0])


def seam_spec(name, shape):
    """``pml_box`` / ``media_mix`` with 264 cells along x: two x tiles of the sweeps, the seam at cell 256, and a body put across it —
    a lossy bar from cell 244 into the x+ layers (pml_box), a Lorentz bar from cell 250 to cell 262 inside it as well (media_mix)."""
    import tidy3d_amd.schema as td
    assert shape[0] == 264
    sim = CASES[name](tuple(shape))
    b = np.asarray(discretize(sim, n_steps=1).spec.boundaries[0])
    assert len(b) - 1 > X_TILE + 8
    x = lambda i: float(b[i])          # noqa: E731
    bodies = [td.Structure(geometry=td.Box(center=(0.5 * (x(244) + x(268)), 0.02, 0.03), size=(x(268) - x(244), 0.3, 0.25)),
                           medium=td.Medium(permittivity=3.0, conductivity=0.02))]
    if name == "media_mix":
        bodies.append(td.Structure(geometry=td.Box(center=(0.5 * (x(250) + x(262)), 0.02, 0.03), size=(x(262) - x(250), 0.2, 0.15)),
                                   medium=td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)])))
    spec = discretize(dataclasses.replace(sim, structures=list(sim.structures) + bodies), n_steps=max(KS)).spec
    spec.decay_every = 0
    for c in range(3):                 # the bodies do cross the seam
        row = spec.mat_idx[c][:, :, X_TILE - 2:X_TILE + 2]
        assert (row > 1).all(axis=2).any(), (name, c)
    return spec


def graded_spec(axis, pmc_min=False):
    """``nonuniform_grid`` with its graded x axis (20 cells, a V profile, CPML) moved to ``axis``; the other graded axis (12 cells,
    a ramp, CPML) and the uniform PEC-walled one follow cyclically.  ``pmc_min``: a PMC wall instead of the layers at the min face
    of the V axis — behind a PEC-backed face the first dual step divides pinned nodes only, behind PMC it divides live ones."""
    import tidy3d_amd.schema as td
    from cases import DL, _sim
    dl_v = tuple(0.03 + 0.02 * np.abs(np.linspace(-1, 1, 20)))
    dl_r = tuple(0.04 + 0.015 * np.linspace(0, 1, 12))
    grids = [td.CustomGrid(dl=dl_v), td.UniformGrid(dl=DL), td.CustomGrid(dl=dl_r)]
    sizes = [float(np.sum(dl_v)), 12 * DL, float(np.sum(dl_r))]
    bnds = [td.Boundary(minus=td.PMCBoundary(), plus=td.PML(num_layers=3)) if pmc_min else td.Boundary.pml(num_layers=3),
            td.Boundary.pec(), td.Boundary.pml(num_layers=3)]
    rot = lambda seq: [seq[(a - axis) % 3] for a in range(3)]          # noqa: E731
    g, s, b = rot(grids), rot(sizes), rot(bnds)
    sim = _sim((1, 1, 1), td.BoundarySpec(x=b[0], y=b[1], z=b[2]), grid_spec=td.GridSpec(grid_x=g[0], grid_y=g[1], grid_z=g[2]))
    spec = discretize(sim.copy(size=tuple(s)), n_steps=max(KS)).spec
    spec.decay_every = 0
    return spec


# label -> builder of the spec: what both modules run beside cases.CASES at their default shapes
SEAM = {"pml_box_x264": lambda: seam_spec("pml_box", (264, 36, 30)), "media_mix_x264": lambda: seam_spec("media_mix", (264, 33, 27))}
TIMES3 = {n + "_x3": (lambda n=n: case_spec(n, times(n))) for n in ("pml_box", "drude_in_pml", "au_array", "lorentz_sphere")}
GRADED = {"graded_x": lambda: graded_spec(0), "graded_y": lambda: graded_spec(1), "graded_z": lambda: graded_spec(2),
          "graded_x_pmc": lambda: graded_spec(0, pmc_min=True)}
BUILDERS = {**{n: (lambda n=n: case_spec(n)) for n in CASES}, **SEAM, **TIMES3, **GRADED}
# label -> axis_shift of the run that must go out in step pairs at K = 6 (FdtdStats.fused2_pairs; the rest keep single steps and say why — their grids are
# too small for a shell, their walls are Bloch / PMC-plus, they run the two-pass kernels): a case that drops out of this list without
# a word would leave the pair kernels untested here
TAKES_PAIRS = {"pec_box": 0, "pec_box_vec": 0, "periodic_box_tall": 0, "pml_box_x264": 0, "media_mix_x264": 0, "pml_box_x3": 0,
               "drude_in_pml_x3": 0, "au_array_x3": 0, "lorentz_sphere_x3": 0, "graded_z": 0, "graded_x": 1, "graded_y": 2}
SHELL2 = ("pml_box_x264", "pml_box_x3", "drude_in_pml_x3", "lorentz_sphere_x3")       # ... and their shells in the shell2 form
_CASES = {}


def case(label, seed=1):
    """the Case of ``label`` (BUILDERS), built once per process: state, references and floors are shared and never changed"""
    if (label, seed) not in _CASES:
        _CASES[(label, seed)] = Case(label, BUILDERS[label](), seed)
    return _CASES[(label, seed)]


# ---------------------------------------------------------------------------------------------------------------- state
def _plane_waves(shape, rng, cplx):
    nz, ny, nx = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = np.zeros(shape, np.complex128 if cplx else np.float64)
    norm = 0.0
    for _ in range(N_WAVES):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        kv = 2.0 * np.pi / rng.uniform(6.0, 16.0) * d
        a = rng.uniform(0.5, 1.0)
        ph = kv[0] * i + kv[1] * j + kv[2] * k
        out += a * np.cos(ph + rng.uniform(0, 2 * np.pi))
        if cplx:
            out += 1j * a * np.cos(ph + rng.uniform(0, 2 * np.pi))
        norm += a
    out /= norm                                             # |.| <= 1 (per part)
    out += NOISE * rng.uniform(-1, 1, size=shape)
    if cplx:
        out += 1j * NOISE * rng.uniform(-1, 1, size=shape)
    return out


def raw_state(spec, seed, amp=AMP):
    """six fp32 (complex64 under Bloch phases) arrays [nz, ny, nx], none of them zero anywhere; E of amplitude ``amp``, H of amp / eta0"""
    nx, ny, nz = spec.shape
    cplx = spec.bloch is not None
    rng = np.random.default_rng([int(seed), nx, ny, nz])
    out = []
    for c in range(6):
        f = (amp if c < 3 else amp / ETA0) * _plane_waves((nz, ny, nx), rng, cplx)
        f = f.astype(np.complex64 if cplx else np.float32)
        tiny = np.float32(1e-3 * (amp if c < 3 else amp / ETA0))
        f[f == 0] = tiny                                    # (a band-limited sum + noise hits 0.0f at no node in practice; make sure)
        out.append(f)
    return out


def mirror_crop(spec):
    """the [z, y, x] slices of what lies inside the PMC-plus walls (``cases.run_case``'s crop)"""
    sl = [slice(None)] * 3
    for a, w in enumerate(getattr(spec, "mirror_plus", None) or ()):
        if w >= 0:
            sl[2 - a] = slice(0, w)
    return tuple(sl)


def _load(o, state):
    for c in range(3):
        o.E[c][...] = state[c]
        o.H[c][...] = state[3 + c]


def admissible_state(spec, seed=1, amp=AMP):
    """-> (state, excluded): the dense state with the pinned nodes and everything beyond a PMC-plus wall at zero, and per component
    the boolean mask of the nodes left out of the measure (those same nodes)."""
    from oracle.fdtd_numpy import OracleFdtd
    state = raw_state(spec, seed, amp)
    o = OracleFdtd(spec)
    _load(o, state)
    o.step()
    inside = mirror_crop(spec)
    excluded = []
    for c in range(6):
        pinned = (o.E[c] if c < 3 else o.H[c - 3]) == 0
        beyond = np.ones(pinned.shape, bool)
        beyond[inside] = False
        ex = pinned | beyond      # (beyond the wall the oracle's step leaves images, not zeros: the crop excludes them)
        state[c] = np.where(ex, 0, state[c]).astype(state[c].dtype)
        excluded.append(ex)
    return state, excluded


def excluded_share(excluded):
    return float(sum(int(m.sum()) for m in excluded)) / float(sum(m.size for m in excluded))


# ---------------------------------------------------------------------------------------------------------------- runs
@dataclasses.dataclass
class Run:
    fields: list                  # six arrays after K steps
    records: dict                 # monitor name -> array
    pairs: int = 0
    shell2_pairs: int = 0
    why: int = 0
    src_paged_pairs: int = 0


def run_oracle(spec, state, K, dtype=np.float64, plant=None, warmup=0):
    """K steps of the oracle from ``state``; ``plant(oracle)`` perturbs the instance before the first step.  ``warmup``: that many
    steps from zero fields first, then the six fields are overwritten with ``state`` (the incident lines, psi and the pole states
    stay as the warm-up left them).  K may be a tuple of ascending counts: -> {K: Run}, every one what a run of its own gives."""
    from oracle.fdtd_numpy import OracleFdtd
    o = OracleFdtd(spec, dtype=dtype)
    if plant is not None:
        plant(o)
    for _ in range(warmup):
        o.step()
    _load(o, state)
    out, done = {}, 0
    for k in ((K,) if np.isscalar(K) else K):
        for _ in range(k - done):
            o.step()
        done = k
        out[k] = Run([np.array(f) for f in o.E + o.H], {n: np.array(v) for n, v in o.results().items()})
    return out[K] if np.isscalar(K) else out


def run_engine(spec, lib, state, K, path, axis_shift=0, twostep=5 + 64 * 3, shell2=1, warmup=0, options=(), **engine_kw):
    """K steps of the library from ``state``: the fused single steps ("fused"), the two-pass kernels ("twopass"), or step pairs
    wherever the run takes them ("pairs": the two-step sweep, shell pairs and the shell2 form forced on as
    tests/test_emu_shell2.py forces them).  ``warmup``: a run of that many steps from zero fields in front of ``set_field`` (the
    counters returned are those of the K steps); ``options``: (key, value) pairs set last; ``engine_kw``: to HipEngine."""
    kw = dict(variant=L.VARIANT_ZMARCH) if path == "twopass" else {}
    with HipEngine(spec, lib=lib, axis_shift=axis_shift, **kw, **engine_kw) as e:
        if path == "pairs":
            e.set_option(L.OPT_TWOSTEP, twostep)
            e.set_option(L.OPT_SHELL_PAIRS, 1)
            e.set_option(L.OPT_SHELL2, shell2)
        else:
            e.set_option(L.OPT_TWOSTEP, 0)
        for key, value in options:
            e.set_option(key, value)
        if warmup:
            e.run(warmup)
        for c in range(6):
            e.set_field(c, state[c])
        st = e.run(K)
        return Run([e.get_field(c) for c in range(6)], e.results(), int(st.fused2_pairs), int(st.shell2_pairs), int(st.fused2_off_reason),
                   int(st.src_paged_pairs))


# ---------------------------------------------------------------------------------------------------------------- measure
def _max3(a):
    """largest value over the 3 x 3 x 3 neighbourhood (last three axes; the edge value repeats beyond the array)"""
    for ax in (-3, -2, -1):
        n = a.shape[ax]
        lo = np.take(a, np.clip(np.arange(n) - 1, 0, n - 1), axis=ax)
        hi = np.take(a, np.clip(np.arange(n) + 1, 0, n - 1), axis=ax)
        a = np.maximum(a, np.maximum(lo, hi))
    return a


def _unit(c):
    return ETA0 if c >= 3 else 1.0


def local_scale(state, ref_fields):
    """[nz, ny, nx]: from the fp64 reference alone — the first step is the state itself"""
    big = np.zeros(ref_fields[0].shape)
    for fields in (state, ref_fields):
        for c in range(6):
            big = np.maximum(big, _unit(c) * np.abs(fields[c]).astype(np.float64))
    rms = np.sqrt(np.mean([np.mean((_unit(c) * np.abs(ref_fields[c])) ** 2) for c in range(6)]))
    return np.maximum(_max3(big), SCALE_FLOOR * rms)


def where(spec, c, kji):
    """what lies at node (k, j, i) of component c, in words"""
    idx = (int(kji[2]), int(kji[1]), int(kji[0]))
    parts = [f"{COMP[c]}[i={idx[0]}, j={idx[1]}, k={idx[2]}] of {tuple(spec.shape)}"]
    for a in range(3):
        N, i, ax = spec.shape[a], idx[a], "xyz"[a]
        for what, lo, hi in (("CPML", spec.pml[a][0].num_layers, spec.pml[a][1].num_layers),
                             ("absorber",) + ((spec.absorber[a][2], spec.absorber[a][3]) if spec.absorber is not None else (0, 0))):
            if i < lo:
                parts.append(f"{ax}- {what} depth {lo - i}/{lo}")
            if i >= N - hi:
                parts.append(f"{ax}+ {what} depth {i - (N - hi) + 1}/{hi}")
        kinds = {0: "PEC", 1: "PMC", 2: "periodic"}
        near = min(i, N - 1 - i)
        if near <= 1:
            side = 0 if i <= N - 1 - i else 1
            parts.append(f"{near} from the {ax}{'-+'[side]} {'wrap' if spec.bc[a][side] == BC_PERIODIC else kinds.get(spec.bc[a][side], '?') + ' wall'}")
        mp = getattr(spec, "mirror_plus", None)
        if mp and mp[a] >= 0 and mp[a] - i <= 2:
            parts.append(f"{mp[a] - i} below the {ax}+ PMC mirror")
    if spec.shape[0] > X_TILE:
        s = idx[0] - X_TILE * round(idx[0] / X_TILE)
        if abs(s) <= 2 and idx[0] >= X_TILE - 2:
            parts.append(f"{s:+d} from the x seam at {X_TILE * round(idx[0] / X_TILE)}")
    if spec.mat_idx is not None:
        m = int(spec.mat_idx[c % 3][idx[2], idx[1], idx[0]])
        nb = spec.mat_idx[c % 3][max(idx[2] - 1, 0):idx[2] + 2, max(idx[1] - 1, 0):idx[1] + 2, max(idx[0] - 1, 0):idx[0] + 2]
        parts.append(f"medium {m} ({getattr(spec.media[m], 'name', '')})" + (", on a body surface" if (nb != m).any() else ""))
    parts += listed(spec, c, idx)
    return "; ".join(parts)


def listed(spec, c, ijk):
    """the source lists that hold node ``ijk`` = (i, j, k) of component c, one clause per list and side: TFSF box or point list, E or
    H side, the entries of that node (index in the list as the spec holds it) of how many, and for a box the aux indices they read"""
    out = []
    side = "EH"[c // 3]
    for n, t in enumerate(spec.tfsf):
        comp, nodes, aux = (t.e_corr_comp, t.e_corr_ijk, t.e_corr_aux) if c < 3 else (t.h_corr_comp, t.h_corr_ijk, t.h_corr_aux)
        hit = np.nonzero((comp == c) & (nodes == np.asarray(ijk)).all(axis=1))[0] if len(comp) else ()
        if len(hit):
            out.append(f"listed: TFSF box {n}, {side} side, entr{'y' if len(hit) == 1 else 'ies'} {', '.join(str(int(q)) for q in hit)} of {len(comp)} "
                       f"({len(hit)} on this node), reading aux {', '.join(str(int(aux[q])) for q in hit)} of the {'h' if c < 3 else 'e'} line")
    for n, s in enumerate(spec.sources):
        hit = np.nonzero((s.comp == c) & (s.ijk == np.asarray(ijk)).all(axis=1))[0] if len(s.comp) else ()
        if len(hit):
            out.append(f"listed: point list {n}{' (' + s.name + ')' if s.name else ''}, {side} side, entr{'y' if len(hit) == 1 else 'ies'} "
                       f"{', '.join(str(int(q)) for q in hit)} of {len(s.comp)} ({len(hit)} on this node)")
    return out


@dataclasses.dataclass
class Worst:
    value: float = 0.0
    comp: str = ""
    index: tuple = ()             # (i, j, k), or the element's index in a record
    at: str = ""

    def __str__(self):
        return f"{self.value:.3e} at {self.at}"


def measure_fields(spec, state, excluded, ref, got):
    """-> per component the worst node: |got - ref| (x eta0 for H) / local scale over every node that is not excluded"""
    scale = local_scale(state, ref.fields)
    out = []
    for c in range(6):
        assert got.fields[c].shape == ref.fields[c].shape, (COMP[c], got.fields[c].shape, ref.fields[c].shape)
        err = _unit(c) * np.abs(got.fields[c].astype(np.complex128) - ref.fields[c]) / scale
        err[excluded[c]] = 0.0
        assert np.isfinite(err).all(), COMP[c]
        kji = np.unravel_index(int(np.argmax(err)), err.shape)
        out.append(Worst(float(err[kji]), COMP[c], (int(kji[2]), int(kji[1]), int(kji[0])), where(spec, c, kji)))
    return out


def measure_records(spec, ref, got):
    """-> per monitor the worst element: |got - ref| / the largest |ref| over the element's 3 x 3 x 3 neighbourhood in the box and the
    monitor's components within the same record (step or frequency), H times eta0, floored at 1e-3 of the record's rms"""
    out = []
    assert set(got.records) == set(ref.records)
    for m in spec.monitors:
        r, g = ref.records[m.name], np.asarray(got.records[m.name])
        assert r.shape == g.shape and r.ndim == 5, (m.name, r.shape, g.shape)
        if r.size == 0:
            continue
        unit = np.asarray([_unit(c) for c in m.comps]).reshape(1, -1, 1, 1, 1)
        a = unit * np.abs(r)
        rms = np.sqrt(np.mean(a ** 2))
        if rms == 0:                                        # (nothing recorded yet: both sides must hold zeros)
            assert not np.abs(g).any(), m.name
            continue
        scale = np.maximum(_max3(a.max(axis=1, keepdims=True)), SCALE_FLOOR * rms)
        err = unit * np.abs(g.astype(np.complex128) - r) / scale
        for a, w in enumerate(getattr(spec, "mirror_plus", None) or ()):        # a box that reaches beyond a PMC-plus wall: the same crop
            if w >= 0 and m.hi[a] > w:
                sl = [slice(None)] * 5
                sl[4 - a] = slice(max(w - m.lo[a], 0), None)
                err[tuple(sl)] = 0.0
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        n, ic, k, j, i = (int(v) for v in at)
        node = (k + m.lo[2], j + m.lo[1], i + m.lo[0])
        out.append(Worst(float(err[at]), COMP[m.comps[ic]], at,
                         f"{m.kind} monitor '{m.name}' record {n}: " + where(spec, m.comps[ic], node)))
    return out


def worst_of(items):
    return max(items, key=lambda w: w.value) if items else Worst()


def measure(spec, state, excluded, ref, got):
    """-> (worst node over the six components, worst record element)"""
    return worst_of(measure_fields(spec, state, excluded, ref, got)), worst_of(measure_records(spec, ref, got))


def rel_l2(ref, got):
    """what the whole-array measure of ``cases.run_case`` sees: the worst over components of |got - ref| / |the whole E resp. H triple|"""
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in ref.fields[:3]))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in ref.fields[3:]))
    return max(float(np.linalg.norm(got.fields[c] - ref.fields[c]) / (en if c < 3 else hn)) for c in range(6))


class Case:
    """A spec with its state, its fp64 references and its fp32 floors per K, computed once and shared by the tests that need them."""
    tag, note, warmup = "dense", "", 0          # (tests/source_state.py: a warm-up in front of the state)

    def __init__(self, label, spec, seed=1):
        self.label, self.spec = label, spec
        self.state, self.excluded = admissible_state(spec, seed)
        self.share = excluded_share(self.excluded)
        self._ref, self._floor = {}, {}

    def ref(self, K):
        if K not in self._ref:
            self._ref[K] = run_oracle(self.spec, self.state, K, warmup=self.warmup)
        return self._ref[K]

    def floor(self, K):
        """(fields, records): the fp32 oracle against the fp64 oracle"""
        if K not in self._floor:
            f, r = measure(self.spec, self.state, self.excluded, self.ref(K), run_oracle(self.spec, self.state, K, dtype=np.float32, warmup=self.warmup))
            self._floor[K] = (f, r)
        return self._floor[K]

    def bar(self, K):
        """one number for the case and K: MARGIN x the larger of the two floors"""
        f, r = self.floor(K)
        return MARGIN * max(f.value, r.value)

    def bars(self, K):
        """(the bar of the nodes, the bar of the record elements): here one number for both"""
        return self.bar(K), self.bar(K)

    def check(self, got, K, what):
        """assert every node and every record element of ``got`` under the bar; -> (fields, records) figures"""
        f, r = measure(self.spec, self.state, self.excluded, self.ref(K), got)
        nbar, rbar = self.bars(K)
        ff, fr = self.floor(K)
        ratio = max(f.value / max(nbar / MARGIN, 1e-300), r.value / max(rbar / MARGIN, 1e-300))
        print(f"[{self.tag}] {self.label} K={K} {what}: nodes {f.value:.3e} records {r.value:.3e} | floor {ff.value:.3e} / {fr.value:.3e} "
              f"bar {nbar:.3e}{'' if rbar == nbar else f' / {rbar:.3e}'} | ratio to floor {ratio:.2f} | excluded {100 * self.share:.2f} %"
              f" | pairs {got.pairs} (shell2 {got.shell2_pairs}, off-reason {got.why}){self.note}")
        assert f.value <= nbar, f"{self.label} K={K} {what}: node over the bar {nbar:.3e} (floor {ff.value:.3e}): {f}"
        assert r.value <= rbar, f"{self.label} K={K} {what}: record over the bar {rbar:.3e} (floor {fr.value:.3e}): {r}"
        return f, r


# ---------------------------------------------------------------------------------------------------------------- planted deviations
REL = 1e-3


def _array_of(o, name, c):
    """the oracle's per-node coefficient array of component c as an array of its own (a scalar or shared table is expanded)"""
    tab = getattr(o, name)
    nx, ny, nz = o.spec.shape
    tab[c] = np.array(np.broadcast_to(tab[c], (nz, ny, nx)), dtype=np.float64)
    return tab[c]


def plant_cb(c, ijk, rel=REL):
    """Cb of E component c at one cell"""
    def plant(o):
        _array_of(o, "cb", c)[ijk[2], ijk[1], ijk[0]] *= 1.0 + rel
    return plant


def plant_pml(axis, name, i, rel=REL):
    """one entry of a CPML table (``c_e``, ``b_h``, ``kinv_e`` ...) of ``axis``: a whole plane of nodes"""
    def plant(o):
        getattr(o.pml[axis], name)[i] *= 1.0 + rel
    return plant


def plant_inv_step(axis, dual, i, rel=REL):
    """1 / primal step (dual=False) or 1 / dual step (dual=True) at index i of ``axis``"""
    def plant(o):
        tab = (o.id if dual else o.ip)[axis]
        tab.reshape(-1)[i] *= 1.0 + rel
    return plant


def plant_absorber(c, ijk, is_h=False, rel=REL):
    """the absorber factor of one node of component c"""
    def plant(o):
        (o.damp_h if is_h else o.damp_e)[c][ijk[2], ijk[1], ijk[0]] *= 1.0 + rel
    return plant


def plant_ade(medium, pole=0, rel=REL):
    """one (kappa, beta) pair of one dispersive medium"""
    def plant(o):
        o.mt.kap[medium][pole] *= 1.0 + rel
        o.mt.bet[medium][pole] *= 1.0 + rel
    return plant
