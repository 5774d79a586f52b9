"""Shared scenarios of the wide-table fused sweep (more than 1023 media through `fused_step_kernel<..., WIDE>`): the grids, the
runs and the comparisons that tests/test_emu_wide_sweep.py (CPU emulator) and tests/test_gpu_wide_sweep.py (device) both use.

The sweep reads 16-bit indices from two words per cell and takes (Ca, Cb) from the table in global memory; row segments whose cells
share one triple of indices <= 1023 keep the packed-word shortcut.  Step pairs are not taken with a wide table
(FDTD_F2_OFF_WIDE_TABLE)."""
import dataclasses
import functools

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

from test_wide_media import DL, wide_sim

TOL = 2e-5                      # the oracle bar of tests/test_wide_media.py: rel-L2 on every record and on all six fields
F2_OFF_WIDE_TABLE = 14          # include/fdtd_hip.h FDTD_F2_OFF_WIDE_TABLE
F2_OFF_VARIANT = 11

PEC = td.Boundary.pec()
SEAM = (264, 24, 16)            # two x tiles (256 + 8 columns): the custom block spans x, the lossy bar sits beside it in the first tile


def _dispersive_bar(size):
    # beside the custom block (its y range ends at -0.15 size_y), clear of the lossy bar's rows
    return td.Structure(geometry=td.Box(center=(0.1 * size[0], -0.2 * size[1], 0), size=(0.3 * size[0], 0.08 * size[1], 0.5 * size[2])),
                        medium=td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)]))


def scenario_sim(name):
    """(a) ... (f) of the issue: one partial x tile with CPML on x / z and PEC + PML on y (38 columns with the layers, padded to 40
    with PEC cells); two x tiles (274 columns, padded to 276); the same inside PEC walls (264 columns, no padding: PML = 0
    instantiations); with layers on x only (PML = 1); nx = 30 between PEC x walls (rows padded to 32 with PEC cells of index 0); a
    Lorentz bar beside the block (an ADE kernel follows the sweep).  (g): the PEC-walled two-tile grid of (c) with rows that are
    uniform along all of x planted into it (PLANTED_WIDE) — the row-segment words beyond the background's."""
    if name == "a":
        return wide_sim((28, 24, 20), 24, eps_span=2.0, sig_span=10.0)
    if name == "b":
        return wide_sim(SEAM, 24, eps_span=2.0, sig_span=10.0)
    if name == "c":
        return wide_sim(SEAM, 24, eps_span=2.0, sig_span=10.0).copy(boundary_spec=td.BoundarySpec(x=PEC, y=PEC, z=PEC))
    if name == "d":
        return wide_sim(SEAM, 24, eps_span=2.0, sig_span=10.0).copy(
            boundary_spec=td.BoundarySpec(x=td.Boundary.pml(num_layers=5), y=PEC, z=PEC))
    if name == "e":
        sim = wide_sim((30, 24, 20), 24, eps_span=2.0, sig_span=10.0)
        return sim.copy(boundary_spec=td.BoundarySpec(x=PEC, y=sim.boundary_spec.y, z=sim.boundary_spec.z))
    if name == "g":
        return scenario_sim("c")
    if name == "f":
        sim = wide_sim((28, 24, 20), 24, eps_span=2.0, sig_span=10.0)
        return sim.copy(structures=list(sim.structures) + [_dispersive_bar(sim.size)])
    raise KeyError(name)


STEPS = {"a": 32, "b": 24, "c": 24, "d": 24, "e": 32, "f": 32, "g": 32}
SCENARIOS = sorted(STEPS)

# Triples of table indices (E_x, E_y, E_z) planted into whole rows — every plane k, every column — that held the background: uniform
# along all of x, so every x tile of such a row is a uniform segment.  plant_rows takes the free interior rows nearest the middle
# row, where the dipoles' fields arrive within the run.  With the WIDE table: a non-background triple of distinct indices <= 1023
# (-> a packed word: a swapped component or a wrong 10-bit shift changes the physics), a triple of indices > 1023 and one with a
# single index > 1023 (-> kMixedWord, the indices read per cell), and a triple at the 10-bit edge.
PLANTED_WIDE = ((2, 3, 4), (1500, 1501, 1502), (2, 3, 1500), (1023, 1022, 1021))
PLANTED_NARROW = ((2, 3, 4), (5, 6, 7), (8, 2, 9), (3, 3, 3))


def plant_rows(spec, triples):
    mat = np.array(spec.mat_idx)                       # [3, nz, ny, nx]
    ny = mat.shape[2]
    free = sorted((j for j in range(1, ny - 1) if np.all(mat[:, :, j, :] == 1)), key=lambda j: (abs(j - ny // 2), j))
    assert len(free) >= len(triples), free
    for j, triple in zip(free, triples):
        assert max(triple) < len(spec.media)
        for c in range(3):
            mat[c, :, j, :] = triple[c]
    return dataclasses.replace(spec, mat_idx=mat)


def segment_classes(spec):
    """How upload_material classifies the 256-cell row segments of `spec` on the device (rows padded to a multiple of 4 with PEC
    cells of index 0 unless x is periodic): numbers of background words, other packed words (one triple, all indices <= 1023),
    uniform segments that name an index > 1023 (kMixedWord by the encoding), and segments whose cells differ.  Restated here so that
    the tests can assert what they cover; the library's own result is what the bit comparisons judge."""
    mat = np.asarray(spec.mat_idx).astype(np.int64)
    nx = mat.shape[3]
    pad = (-nx) % 4 if spec.bc[0][1] != 2 else 0
    if pad:
        mat = np.concatenate([mat, np.zeros(mat.shape[:3] + (pad,), np.int64)], axis=3)
    out = {"background": 0, "packed": 0, "uniform_wide_index": 0, "mixed": 0}
    for i0 in range(0, mat.shape[3], 256):
        seg = mat[:, :, :, i0:i0 + 256]
        uniform = np.all(seg == seg[..., :1], axis=(0, 3))
        first = seg[..., 0]
        small = np.all(first <= 1023, axis=0)
        bg = uniform & np.all(first == 1, axis=0)
        out["background"] += int(bg.sum())
        out["packed"] += int((uniform & small & ~bg).sum())
        out["uniform_wide_index"] += int((uniform & ~small).sum())
        out["mixed"] += int((~uniform).sum())
    return out


@functools.lru_cache(maxsize=None)
def scenario(name):
    disc = discretize(scenario_sim(name), n_steps=STEPS[name])
    assert 1023 < len(disc.spec.media) < 65531, (name, len(disc.spec.media))
    if name == "g":
        assert disc.spec.shape[0] % 4 == 0 and disc.spec.shape[0] > 256
        disc = dataclasses.replace(disc, spec=plant_rows(disc.spec, PLANTED_WIDE))
        cls = segment_classes(disc.spec)
        nz = disc.spec.shape[2]
        # two x tiles per planted row and plane: two rows packed, two rows uniform with an index > 1023
        assert cls["packed"] == 2 * 2 * nz and cls["uniform_wide_index"] == 2 * 2 * nz and cls["mixed"] > 0, cls
    return disc


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(records, E, H) of the fp64 oracle: computed once per scenario and left unchanged."""
    from oracle.fdtd_numpy import OracleFdtd
    o = OracleFdtd(scenario(name).spec)
    ref = o.run()
    return ref, [np.array(x) for x in o.E], [np.array(x) for x in o.H]


@dataclasses.dataclass
class Out:
    fields: list
    records: dict
    stats: object
    variant: int


def run(spec, lib, variant=L.VARIANT_FUSED, options=None, flags=L.FLAG_TIME_KERNELS, **kw):
    with HipEngine(spec, lib=lib, variant=variant, flags=flags, **kw) as e:
        for k, v in (options or {}).items():
            e.set_option(k, v)
        st = e.run()
        assert not st.diverged
        return Out([e.get_field(c) for c in range(6)], {k: np.asarray(v) for k, v in e.results().items()}, st, e.variant)


def assert_fused_wide(out, n_steps):
    """the single-step fused sweep ran every step (kernel timing on: the launches are counted), nothing two-pass, no step pairs"""
    st = out.stats
    assert out.variant == L.VARIANT_FUSED
    assert st.fused_kernel_launches >= n_steps and st.h_kernel_launches == 0 and st.e_kernel_launches == 0, \
        (st.fused_kernel_launches, st.h_kernel_launches, st.e_kernel_launches)
    assert st.fused2_pairs == 0 and st.shell_pairs == 0 and st.shell2_pairs == 0 and st.two_step_pairs == 0
    assert st.fused2_off_reason in (F2_OFF_WIDE_TABLE, 1), st.fused2_off_reason        # (1: pairs switched off by the caller)


def assert_oracle(out, name):
    ref, E, H = oracle(name)
    scale = max(np.linalg.norm(v) / np.sqrt(v.size) for v in ref.values())
    for k in ref:
        den = max(np.linalg.norm(ref[k]), 0.5 * scale * np.sqrt(ref[k].size))
        err = np.linalg.norm(out.records[k] - ref[k]) / den
        print(f"[wide sweep] {name} record {k}: rel-L2 {err:.3e}")
        assert err < TOL, (name, k, err)
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in E))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in H))
    assert en > 0
    for c in range(3):
        ee, eh = np.linalg.norm(out.fields[c] - E[c]) / en, np.linalg.norm(out.fields[3 + c] - H[c]) / hn
        print(f"[wide sweep] {name} E{c} {ee:.3e} H{c} {eh:.3e}")
        assert ee < TOL and eh < TOL, (name, c, ee, eh)


def assert_same_bits(a, b, what):
    for c in range(6):
        assert np.array_equal(a.fields[c], b.fields[c]), (what, "field", c, float(np.abs(a.fields[c] - b.fields[c]).max()))
    assert set(a.records) == set(b.records)
    for k in a.records:
        assert np.array_equal(a.records[k], b.records[k]), (what, "record", k)


# ---- the same problem under a narrow and a wide table ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_spec(kind="layers", n_steps=32):
    """fewer than 1000 media: one coarsening step keeps these data in the narrow table (tests/test_wide_media.py).
    "layers": wide_sim((28, 24, 20), 24) as it stands — 38 columns with the x layers, padded to 40, so every row ends in PEC cells and
    EVERY segment is mixed, under any table.  "planted": the same data between PEC x walls (28 columns, no padding) with x-uniform
    rows of non-background triples planted (PLANTED_NARROW): under a table that is only padded these keep packed words beside the
    background's; remapped above 1023 they become uniform segments that name wide indices."""
    sim = wide_sim((28, 24, 20), 24)
    if kind == "planted":
        sim = sim.copy(boundary_spec=td.BoundarySpec(x=PEC, y=sim.boundary_spec.y, z=sim.boundary_spec.z))
    spec = discretize(sim, n_steps=n_steps).spec
    assert 12 < len(spec.media) < 1000, len(spec.media)
    if kind == "planted":
        assert spec.shape[0] % 4 == 0
        spec = plant_rows(spec, PLANTED_NARROW)
    return spec


def widened(spec, n_table, first=None):
    """`spec` with its table padded to `n_table` entries (copies of the background medium, unused).  `first`: every used index >= 2
    moves to first, first + 1, ... — index 0 (PEC) and 1 (background) stay — so that no segment with a body keeps a packed word."""
    n = len(spec.media)
    perm = np.arange(n)
    if first is not None:
        perm[2:] = first + np.arange(n - 2)
        assert first >= 1024 and first + n - 2 <= n_table
    media = [spec.media[1]] * n_table
    for i in range(n):
        media[perm[i]] = spec.media[i]
    return dataclasses.replace(spec, media=media, mat_idx=perm[spec.mat_idx].astype(np.uint16))


WIDENED = {"padded to 1100": (1100, None), "remapped to 2000+": (40000, 2000), "remapped to 33000+": (40000, 33000)}
SINGLE_STEPS = {L.OPT_TWOSTEP: 0, L.OPT_SHELL_PAIRS: 0}


# ---- lifecycle ------------------------------------------------------------------------------------------------------------
def lifecycle(lib, name="a"):
    """one handle: run, reset, run again -> the same bits; get_field / set_field half way -> the bits of a fresh handle's full run"""
    spec = scenario(name).spec
    n = STEPS[name]
    fresh = run(spec, lib)
    with HipEngine(spec, lib=lib, variant=L.VARIANT_FUSED) as e:
        e.run()
        first = [e.get_field(c) for c in range(6)]
        rec1 = {k: np.asarray(v) for k, v in e.results().items()}
        e.reset()
        e.run()
        second = [e.get_field(c) for c in range(6)]
        rec2 = {k: np.asarray(v) for k, v in e.results().items()}
        for c in range(6):
            assert np.array_equal(first[c], second[c]) and np.array_equal(first[c], fresh.fields[c]), c
        for k in rec1:
            assert np.array_equal(rec1[k], rec2[k]) and np.array_equal(rec1[k], fresh.records[k]), k
        # half way: read the state out, write it back, go on
        e.reset()
        e.run(n // 2)
        mid = [e.get_field(c) for c in range(6)]
        for c in range(6):
            e.set_field(c, mid[c])
        e.run(n - n // 2)
        for c in range(6):
            assert np.array_equal(e.get_field(c), fresh.fields[c]), ("get/set mid-run", c)
        assert e.stats().fused2_pairs == 0
