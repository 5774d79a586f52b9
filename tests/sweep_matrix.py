"""The scenario matrix that reaches every listed instantiation of the two-step sweep, fused2_step_kernel<LB, OPT> (the table
FDTD_F2_LIST_ALL of tidy3d_amd/csrc/fdtd_fused2.hpp, read back through fdtd_sweep_table).  Shared by tests/test_emu_sweep_table.py
(CPU emulator) and tests/test_gpu_sweep_table.py (device): plain functions, no fixtures.

One SCENARIO per combination of features that set OPT bits:

    kF2Mat    a lossy bar through the seam column 256, a sub-pixel sphere and a PEC box
    kF2Mon    an interval-1 probe (E_x, H_y, H_z) with a node in the column left of the seam, plus a DFT plane
    kF2Damp   absorber layers on all faces
    kF2Clip   CPML walls with FDTD_OPT_SHELL_PAIRS = 1 (the sweep covers the bulk of the shell pair)
    kF2Disp   a Lorentz sphere on the seam, advanced inside the pairs
    kF2Src    a current sheet of more than kMaxInj nodes across the whole cross-section (paged source terms)

and per scenario VARIANTS (W, nt, defer): waves per workgroup (the launch bound: <= 8 -> 512, <= 12 -> 768, else 1024 threads;
dispersive and paged-source words have no 768 form), FDTD_OPT_MEM_HINTS (kF2NT) and FDTD_OPT_SEAM_DEFER (kF2Rep: the sweeps behind
the first pair of a run read the repair array — sixteen waves, or any W with the testing value 2).  A variant DECLARES the set of
(LB, OPT, W) its run launches; check_scenario holds the run to single steps of the same library bit for bit and to that set exactly
(fdtd_get_sweep_words), so a case that falls onto a neighbouring instantiation fails.  Once per scenario a pairs run is held to the
fp64 oracle at the project's bar.

Shapes: every grid has one seam with a ragged second x tile; rows and planes are chosen so that at every W used the launch has
two or more tile rows with a ragged last one (R = W - 3 rows are written per workgroup) and every chunk length leaves a ragged last
chunk."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

from test_emu_fused2 import DL, PEC, PULSE

# the OPT word (fdtd_fused2.hpp)
NT, MAT, MON, DAMP, CLIP, DISP, SRC, REP = 1, 2, 4, 8, 16, 32, 64, 8192
WHATIF_SHIFT, WHATIF_MASK = 8, 15
BIT_NAMES = ((NT, "nt"), (MAT, "mat"), (MON, "mon"), (DAMP, "damp"), (CLIP, "clip"), (DISP, "disp"), (SRC, "src"), (REP, "rep"))

ORACLE_BAR = 2e-5               # cases.run_case: rel-L2 of every record and of the final E / H triples, fp32 against the fp64 oracle
RUNS = (11, 15)                 # two fdtd_run calls, the second starting on an odd step: 5 + 7 pairs and a single step each
PAIRS = sum(r // 2 for r in RUNS)

ABS = td.BoundarySpec.all_sides(td.Absorber(num_layers=3))
PML = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary.pml(num_layers=3), z=td.Boundary.pml(num_layers=3))
LAYERS = {"pec": (0, 0, 0), "abs": (3, 3, 3), "pml": (4, 3, 3)}        # per face; they lie outside the simulation's own box
LOR = td.Lorentz(eps_inf=2.0, coeffs=[(2.0, 4e14, 2e13)])

# (shapes of the grid on the device, layers included)
# whole grid: 31 rows = 6 x 5 + 1 (8 waves), 3 x 9 + 4 (12), 2 x 13 + 5 (16), 15 x 2 + 1 (5); 12 planes
WHOLE = (264, 31, 12)
# CPML (4 / 3 / 3 layers): the bulk of the shell pair is [lo + 2, hi - 1) per axis — 17 rows = 3 x 5 + 2, 9 + 8, 13 + 4, 8 x 2 + 1; 11 planes
SHELL = (300, 26, 20)
# chunk lengths per W with a ragged last chunk on 12 planes (whole grid) / 11 planes (bulk)
ZC = {False: {5: 5, 8: 5, 12: 7, 16: 8}, True: {5: 3, 8: 4, 12: 7, 16: 6}}


def lb_of(w: int, opt: int) -> int:
    """the launch bound that serves `w` waves (fused2_lb)"""
    if opt & REP:
        return 1024
    if w <= 8:
        return 512
    return 768 if (w <= 12 and not opt & (SRC | DISP)) else 1024


def word_name(opt: int) -> str:
    wv = (opt >> WHATIF_SHIFT) & WHATIF_MASK
    return "+".join(n for b, n in BIT_NAMES if opt & b) + (f"+whatif{wv}" if wv else "") or "plain"


@dataclasses.dataclass(frozen=True)
class Scenario:
    name: str
    media: str = "vac"            # "vac", "mat" (kF2Mat) or "disp" (kF2Mat | kF2Disp)
    mon: bool = False             # kF2Mon
    walls: str = "pec"            # "pec", "abs" (kF2Damp) or "pml" (kF2Clip)
    sheet: bool = False           # kF2Src (| kF2Mon | kF2NT)
    variants: Tuple[Tuple[int, int, int], ...] = ()        # (W, nt, defer)

    @property
    def shell(self) -> bool:
        return self.walls == "pml"

    @property
    def shape(self) -> Tuple[int, int, int]:
        return SHELL if self.shell else WHOLE

    def opt(self, nt: int) -> int:
        """the word of a launch without the repair array (fused2_opt)"""
        o = (NT if nt else 0) | (MAT if self.media != "vac" else 0) | (MON if self.mon else 0)
        o |= {"pec": 0, "abs": DAMP, "pml": CLIP}[self.walls]
        if self.media == "disp":
            o |= DISP | NT
        if self.sheet:
            o |= SRC | MON | NT
        return o

    def words(self, w: int, nt: int, defer: int) -> frozenset:
        """the (LB, OPT, W) a run of this variant launches: with deferred seam repair the first pair of each fdtd_run reads the
        fields (the plain word at W's own launch bound), the others the repair array (kF2Rep, the sixteen-wave instantiation)"""
        o = self.opt(nt)
        out = {(lb_of(w, o), o, w)}
        if defer:
            out.add((lb_of(w, o | REP), o | REP, w))
        return frozenset(out)


def _full(ws=(8, 12, 16), nts=(0, 1)):
    return tuple((w, nt, 0) for w in ws for nt in nts)


def _scenarios() -> List[Scenario]:
    out = []
    # base + deferred-seam lists: whole grid, PEC walls / absorber layers, every (mat, mon, nt) at 512 / 768 / 1024; the words without
    # the monitor table also with deferred seam repair at sixteen waves.  Five waves: once in the base list, once (testing value 2 of
    # FDTD_OPT_SEAM_DEFER: the sixteen-wave instantiation at another workgroup size) in the deferred-seam list
    for walls in ("pec", "abs"):
        for media in ("vac", "mat"):
            for mon in (False, True):
                v = _full()
                if not mon:
                    v += ((16, 0, 1), (16, 1, 1))
                if walls == "pec" and media == "mat" and mon:
                    v += ((5, 1, 0),)
                if walls == "abs" and media == "mat" and not mon:
                    v += ((5, 1, 2),)
                out.append(Scenario(f"{walls}_{media}{'_mon' if mon else ''}", media, mon, walls, False, v))
    # clipped list: CPML walls, every (mat, mon, nt) at 512 / 768 / 1024
    for media in ("vac", "mat"):
        for mon in (False, True):
            v = _full() + (((5, 1, 0),) if media == "mat" and mon else ())
            out.append(Scenario(f"pml_{media}{'_mon' if mon else ''}", media, mon, "pml", False, v))
    # dispersive list (non-temporal stores always; 512 and 1024 — twelve waves run the 1024 form)
    for walls in ("pec", "abs", "pml"):
        for mon in (False, True):
            v = ((8, 1, 0), (16, 1, 0)) + (((5, 1, 0), (12, 1, 0)) if walls == "pec" and mon else ())
            out.append(Scenario(f"{walls}_disp{'_mon' if mon else ''}", "disp", mon, walls, False, v))
    # paged-source list (monitor table and non-temporal stores always)
    for walls in ("pec", "abs", "pml"):
        for media in ("vac", "mat", "disp"):
            v = ((8, 1, 0), (16, 1, 0)) + (((5, 1, 0), (12, 1, 0)) if walls == "pml" and media == "mat" else ())
            out.append(Scenario(f"{walls}_{media}_sheet", media, False, walls, True, v))
    return out


SCENARIOS: Dict[str, Scenario] = {s.name: s for s in _scenarios()}


def declared_pairs() -> Dict[Tuple[int, int], List[str]]:
    """(LB, OPT) -> the cases ("scenario[W, nt, defer]") that declare — and, passing, have launched and bit-checked — it"""
    out: Dict[Tuple[int, int], List[str]] = {}
    for s in SCENARIOS.values():
        for (w, nt, defer) in s.variants:
            for (lb, opt, _) in sorted(s.words(w, nt, defer)):
                out.setdefault((lb, opt), []).append(f"{s.name}[W={w} nt={nt} defer={defer}]")
    return out


def build_sim(s: Scenario) -> td.Simulation:
    N = s.shape
    size = tuple((n - 2 * l - 1e-6) * DL for n, l in zip(N, LAYERS[s.walls]))
    x0 = -0.5 * size[0]                      # the x-min face of the simulation's box
    xs = (256 - 0.5 * N[0]) * DL             # the seam: column 256 of the grid is the first of the second x tile
    # electric dipoles only (magnetic nodes keep single steps with absorber layers, and set kF2Mon by themselves): two deep inside, one ON
    # column 255 and one between columns 256 and 257; without CPML also next to both x walls (inside a shell they would stop its pairs)
    srcs = [td.PointDipole(center=(0.02, 0.01, 0.03), source_time=PULSE, polarization="Ez"),
            td.PointDipole(center=(-0.11, 0.06, -0.05), source_time=PULSE, polarization="Ex"),
            td.PointDipole(center=(xs - 1.0 * DL, -0.05, 0.04), source_time=PULSE, polarization="Ey"),
            td.PointDipole(center=(xs + 0.5 * DL, 0.0, 0.0), source_time=PULSE, polarization="Ex")]
    if not s.shell:
        srcs += [td.PointDipole(center=(x0 + 2.3 * DL, 0.03, 0.02), source_time=PULSE, polarization="Ez"),
                 td.PointDipole(center=(-x0 - 3.2 * DL, 0.1, -0.07), source_time=PULSE, polarization="Ey")]
    if s.sheet:                              # nx * nz nodes, through the seam and (absorber, CPML) through the layers
        srcs.append(td.UniformCurrentSource(center=(0, 0.2, 0), size=(td.inf, 0, td.inf), source_time=PULSE, polarization="Ex"))
    structures = []
    if s.media != "vac":
        structures = [td.Structure(geometry=td.Box(center=(xs, 0, 0), size=(1.0, 0.3, 0.2)), medium=td.Medium(permittivity=3.0, conductivity=0.02)),
                      td.Structure(geometry=td.Sphere(center=(0.3, 0.1, 0), radius=0.22), medium=td.Medium(permittivity=2.5)),
                      td.Structure(geometry=td.Box(center=(-0.4, -0.1, 0.05), size=(0.1, 0.1, 0.1)), medium=td.PEC)]
    if s.media == "disp":                    # (inside a shell: three and more cells inside the bulk)
        structures.append(td.Structure(geometry=td.Sphere(center=(xs + 0.05, 0, 0), radius=0.2), medium=LOR))
    mons = []
    if s.mon:
        mons = [td.FieldTimeMonitor(center=(xs - 0.6 * DL, 0.0, 0.05), size=(0, 0, 0), name="seam", interval=1,
                                    fields=["Ex", "Hy", "Hz"], colocate=False),
                td.FieldMonitor(center=(0, 0, 0.02), size=(td.inf, td.inf, 0), freqs=[3e14], name="f", colocate=False)]
    bspec = {"pec": PEC, "abs": ABS, "pml": PML}[s.walls]
    return td.Simulation(size=size, grid_spec=td.GridSpec.uniform(dl=DL), run_time=1e-12, sources=srcs, structures=structures,
                         monitors=mons, boundary_spec=bspec, shutoff=0)


def build_spec(s: Scenario):
    disc = discretize(build_sim(s), n_steps=sum(RUNS))
    disc.spec.decay_every = 0
    assert tuple(disc.spec.shape) == s.shape, disc.spec.shape
    return disc.spec


@dataclasses.dataclass
class Run:
    fields: list
    records: dict
    pairs: int
    shell2_pairs: int
    disp_pairs: int
    src_pairs: int
    words: frozenset


def initial_fields(shape, seed: int = 7):
    """random initial fields (E_x .. H_z): every tile, seam and layer carries data from the first step on"""
    rng = np.random.default_rng(seed)
    return [((1e-3 if c < 3 else 1e-3 / 376.73) * rng.uniform(-1, 1, size=shape)).astype(np.float32) for c in range(6)]


def run(spec, lib, s: Scenario, emu: bool, w: int = 0, nt: int = 1, defer: int = 0) -> Run:
    """w = 0: single steps (the reference)"""
    zc = ZC[s.shell].get(w, 0)
    kw = dict(z_chunk=2) if emu else {}
    with HipEngine(spec, lib=lib, variant=L.VARIANT_FUSED, **kw) as e:
        if emu:
            e.set_option(L.OPT_ROWS, 3)
        else:
            e.set_option(L.OPT_PLACEMENT_TRIES, 0)
        e.set_option(L.OPT_TWOSTEP, w + 64 * zc if w else 0)
        e.set_option(L.OPT_MEM_HINTS, nt)
        e.set_option(L.OPT_SEAM_DEFER, defer)
        if s.shell:
            e.set_option(L.OPT_PML_SPLIT, 1)
            e.set_option(L.OPT_SHELL_PAIRS, 1)
            e.set_option(L.OPT_SHELL2, 1)
        for c, f in enumerate(initial_fields(e.get_field(0).shape)):
            e.set_field(c, f)
        out = Run([], {}, 0, 0, 0, 0, frozenset())
        for r in RUNS:
            st = e.run(r)
            out.pairs += int(st.fused2_pairs)
            out.shell2_pairs += int(st.shell2_pairs)
            out.disp_pairs += int(st.disp_pairs)
            out.src_pairs += int(st.src_paged_pairs)
        out.fields = [e.get_field(c) for c in range(6)]
        out.records = {k: np.asarray(v) for k, v in e.results().items()}
        out.words = frozenset(e.sweep_words())
        return out


def oracle_deviation(spec, got: Run) -> float:
    """cases.run_case's figure — the worst rel-L2 over the records and the final E / H triples — with the oracle started from the
    run's initial fields"""
    from oracle.fdtd_numpy import OracleFdtd
    o = OracleFdtd(spec)
    for c, f in enumerate(initial_fields(got.fields[0].shape)):
        (o.E if c < 3 else o.H)[c % 3][...] = f
    ref = o.run()
    worst = 0.0
    scale = max(np.linalg.norm(v) / np.sqrt(v.size) for v in ref.values()) if ref else 1.0
    for k in ref:
        den = max(np.linalg.norm(ref[k]), 0.5 * scale * np.sqrt(ref[k].size), 1e-300)
        worst = max(worst, float(np.linalg.norm(got.records[k] - ref[k]) / den))
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.E))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.H))
    assert en > 0 and hn > 0
    for c in range(3):
        worst = max(worst, float(np.linalg.norm(got.fields[c] - o.E[c]) / en))
        worst = max(worst, float(np.linalg.norm(got.fields[3 + c] - o.H[c]) / hn))
    return worst


def check_scenario(name: str, lib, emu: bool, launched: Dict[Tuple[int, int], List[str]]):
    """One reference (single steps, a fresh handle) shared by the scenario's variants; every variant: pairs, bits, words.  The pairs a
    passing variant launched go into `launched` ((LB, OPT) -> cases).  The first variant's run is held to the oracle too.  Failures of all variants are reported."""
    s = SCENARIOS[name]
    spec = build_spec(s)
    ref = run(spec, lib, s, emu)
    assert ref.pairs == 0 and ref.shell2_pairs == 0 and not ref.words, (ref.pairs, ref.words)
    assert min(float(np.abs(f).max()) for f in ref.fields) > 0
    if s.mon:
        assert set(ref.records) == {"seam", "f"}
    for k, v in ref.records.items():
        assert float(np.abs(v).max()) > 0, k
    failures = []
    first = None
    for (w, nt, defer) in s.variants:
        case = f"{name}[W={w} nt={nt} defer={defer}]"
        got = run(spec, lib, s, emu, w, nt, defer)
        first = first or got
        bad = []
        if got.pairs != PAIRS or (s.shell and got.shell2_pairs != PAIRS) or (s.media == "disp" and got.disp_pairs != PAIRS) or \
                (s.sheet and got.src_pairs != PAIRS):
            bad.append(f"pairs {got.pairs}, shell2 {got.shell2_pairs}, dispersive {got.disp_pairs}, paged-source {got.src_pairs}: expected {PAIRS}")
        for c in range(6):
            if not np.array_equal(got.fields[c], ref.fields[c]):
                bad.append(f"field {c}: {int((got.fields[c] != ref.fields[c]).sum())} cells differ, max {float(np.abs(got.fields[c] - ref.fields[c]).max()):.3e}")
        if set(got.records) != set(ref.records):
            bad.append(f"records {sorted(got.records)}")
        for k in ref.records:
            if k in got.records and not np.array_equal(got.records[k], ref.records[k]):
                bad.append(f"record {k} differs")
        want = s.words(w, nt, defer)
        if got.words != want:
            bad.append("launched " + ", ".join(f"({lb}, {word_name(o)}, {ww})" for lb, o, ww in sorted(got.words)) +
                       "; written to reach " + ", ".join(f"({lb}, {word_name(o)}, {ww})" for lb, o, ww in sorted(want)))
        if bad:
            failures.append(case + ": " + "; ".join(bad))
        else:
            for (lb, opt, _) in got.words:
                launched.setdefault((lb, opt), []).append(case)
    # the oracle, once: the pairs run of the scenario's first variant
    dev = oracle_deviation(spec, first)
    print(f"sweep table: {name}: worst deviation from the fp64 oracle {dev:.3e} (bar {ORACLE_BAR:g})")
    if not dev < ORACLE_BAR:
        failures.append(f"{name}: {dev:.3e} from the oracle")
    assert not failures, "\n".join(failures)
    return dev


# Listed pairs that no option setting reaches: (LB, OPT) -> the line of launch_fused2 / fused2_opt that keeps it out.  (None found: every
# word fused2_words_instantiated forms is also formed by a scenario above.)
UNREACHABLE: Dict[Tuple[int, int], str] = {}


def check_table(lib, launched: Optional[Dict[Tuple[int, int], List[str]]] = None):
    """The closing condition: every listed (LB, OPT) but the what-if words and UNREACHABLE is declared by a case of the matrix — whose
    own assertions hold its run to exactly the declared words — and no case declares a pair the table lacks.  `launched` (the cases of
    this process that passed): a case recorded there must agree with its declaration.  Prints the table with its cases."""
    table = lib.sweep_table()
    assert len(set(table)) == len(table)
    declared = declared_pairs()
    lines, missing = [], []
    for (lb, opt) in table:
        if (opt >> WHATIF_SHIFT) & WHATIF_MASK:
            lines.append(f"  ({lb:4d}, 0x{opt:04x} {word_name(opt)}): what-if word, out of scope")
            continue
        if (lb, opt) in UNREACHABLE:
            lines.append(f"  ({lb:4d}, 0x{opt:04x} {word_name(opt)}): unreachable — {UNREACHABLE[(lb, opt)]}")
            assert (lb, opt) not in declared
            continue
        cases = declared.get((lb, opt), [])
        ran = set((launched or {}).get((lb, opt), []))
        lines.append(f"  ({lb:4d}, 0x{opt:04x} {word_name(opt)}): " + ", ".join(c + ("*" if c in ran else "") for c in cases))
        if not cases:
            missing.append((lb, hex(opt), word_name(opt)))
    print("sweep table: (LB, OPT) -> the cases that launch it (* = launched and bit-checked in this process)")
    print("\n".join(lines))
    assert not missing, f"listed instantiations without a case: {missing}"
    extra = sorted(set(declared) - set(table))
    assert not extra, f"cases written to reach pairs the table lacks: {extra}"
    for pair in UNREACHABLE:
        assert pair in table, pair
    if launched:
        for pair, cases in launched.items():
            assert pair in declared and set(cases) <= set(declared[pair]), (pair, cases)
    return table
