"""Deferred seam repair (FDTD_OPT_SEAM_DEFER) on the device: the sixteen-wave sweeps the large runs take, at grid sizes the
emulator cases do not reach — three x tiles with a short last one, materials through a seam, absorber layers — with the option
on, off and with single steps: the same bits.  tests/test_emu_seam_defer.py has the cases proper."""
import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

from cases import DL, PULSE

pytestmark = pytest.mark.gpu

N = (520, 96, 72)


def _sim(structures=(), bspec=None):
    sx, sy, sz = (n * DL for n in N)
    bspec = bspec or td.BoundarySpec.all_sides(td.PECBoundary())
    srcs = [td.PointDipole(center=(-0.5 * sx + 255.0 * DL, 0.13, 0.07), source_time=PULSE, polarization="Ey"),     # on column 255
            td.PointDipole(center=(-0.5 * sx + 256.5 * DL, -0.2, 0.3), source_time=PULSE, polarization="Ex"),
            td.PointDipole(center=(-0.5 * sx + 512.0 * DL, 0.4, -0.5), source_time=PULSE, polarization="Ez"),      # on column 512
            td.PointDipole(center=(0.3, -1.2, 1.1), source_time=PULSE, polarization="Ez")]
    return td.Simulation(size=(sx, sy, sz), grid_spec=td.GridSpec.uniform(dl=DL), run_time=1e-12, structures=list(structures),
                         sources=srcs, monitors=[], boundary_spec=bspec, shutoff=0)


def _run(spec, lib, twostep, defer, runs=(21, 30)):
    with HipEngine(spec, lib=lib, variant=L.VARIANT_FUSED) as e:
        e.set_option(L.OPT_PLACEMENT_TRIES, 0)
        e.set_option(L.OPT_TWOSTEP, twostep)
        e.set_option(L.OPT_SEAM_DEFER, defer)
        deferred = flushes = 0
        for r in runs:
            e.run(r)
            ss = e.seam_stats()
            assert int(ss.seam_pending) == 0
            deferred += int(ss.seam_deferred_pairs)
            flushes += int(ss.seam_flushes)
        return [e.get_field(c) for c in range(6)], deferred, flushes


BAR = [td.Structure(geometry=td.Box(center=(-1.0, 0, 0), size=(8.0, 0.8, 0.6)), medium=td.Medium(permittivity=3.0, conductivity=0.02)),
       td.Structure(geometry=td.Sphere(center=(12.7, 0.1, 0), radius=0.9), medium=td.Medium(permittivity=2.5))]
ABS = td.BoundarySpec(x=td.Boundary.absorber(num_layers=6), y=td.Boundary(minus=td.PECBoundary(), plus=td.Absorber(num_layers=4)),
                      z=td.Boundary.absorber(num_layers=4))


@pytest.mark.parametrize("name", ["vacuum", "materials", "absorber"])
def test_deferred_pairs_equal_stored_pairs_and_single_steps(name, hip_lib):
    sim = _sim(structures=BAR if name == "materials" else (), bspec=ABS if name == "absorber" else None)
    disc = discretize(sim, n_steps=51)
    disc.spec.decay_every = 0
    ref, d0, _ = _run(disc.spec, hip_lib, 0, 0)
    off, d1, f1 = _run(disc.spec, hip_lib, 16 + 64 * 32, 0)
    on, d2, f2 = _run(disc.spec, hip_lib, 16 + 64 * 32, 1)
    assert d0 == 0 and d1 == 0 and f1 == 0 and f2 == 0
    assert d2 == 9 + 14, d2                    # runs of 21 and 30 steps: 10 + 15 pairs, all but the last of each deferred
    assert max(float(np.abs(f).max()) for f in ref) > 0
    for c in range(6):
        assert np.array_equal(off[c], ref[c]), c
        assert np.array_equal(on[c], ref[c]), c


@pytest.mark.parametrize("name", ["vacuum", "materials", "absorber"])
def test_flush_in_front_of_a_paged_source_pair(name, hip_lib):
    """The first source list ends at step 10, the others go on: the pair of steps 10, 11 carries paged source terms, which the
    instantiation that reads the repair array does not — the deferred pair in front of it is flushed (seam_flush_kernel).  Pairs
    0 ... 4 deferred, one flush."""
    sim = _sim(structures=BAR if name == "materials" else (), bspec=ABS if name == "absorber" else None)
    disc = discretize(sim, n_steps=30)
    disc.spec.decay_every = 0
    sc = disc.spec.sources[0]
    sc.wave_e, sc.wave_h = np.asarray(sc.wave_e)[:10].copy(), np.asarray(sc.wave_h)[:10].copy()
    ref, _, _ = _run(disc.spec, hip_lib, 0, 0, runs=(30,))
    on, d, f = _run(disc.spec, hip_lib, 16 + 64 * 32, 1, runs=(30,))
    assert d == 5 and f == 1, (d, f)
    for c in range(6):
        assert np.array_equal(on[c], ref[c]), c
