"""Exact projection (far_field_approx=False) with its surface integrals on the device: ``fdtd_near_field`` (kernel K9b,
csrc/fdtd_near_field.hpp), here compiled for the host by tests/hipemu, against the longdouble reference of
tests/exact_projection_case.py — held to 8 x the floor the host path's own float64 arithmetic leaves against that reference —
and ``web.run(..., exact_projection_device=...)`` / ``data.assemble`` end to end.

Floors and the emulator's worst ratios as measured (printed by the tests; docs/history/EXACT_PROJECTION.md carries the table)."""
import ctypes

import numpy as np
import pytest

from tidy3d_amd import projection, web
from tidy3d_amd.data import assemble
from tidy3d_amd.discretize import discretize
from tidy3d_amd.exceptions import SolverLibraryError

import exact_projection_case as xc
from flux_time_case import run_engine


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_twelve_sums_within_eight_floors(emu_lib, name):
    xc.check_case(emu_lib, name, "emulator")


def test_chunk_counts_on_either_side_of_every_threshold(emu_lib):
    for name, want in xc.CHUNKS.items():
        n_u, n_v, n_pts = xc.CASES[name][:3]
        assert emu_lib.near_field_chunks(n_pts, n_u, n_v) == want, name
    # the rule is a function of n_pts and n_u * n_v alone
    assert emu_lib.near_field_chunks(127, 91, 91) == emu_lib.near_field_chunks(127, 8281, 1) == emu_lib.near_field_chunks(1, 91, 91)
    assert emu_lib.near_field_chunks(1 << 20, 256, 256) == 1 and emu_lib.near_field_chunks(1, 256, 256) == 64
    assert emu_lib.near_field_chunks(128, 256, 256) == emu_lib.near_field_chunks(1023, 256, 256) == 8


def test_two_calls_give_equal_bits(emu_lib):
    for name in ("l37x29_near_real", "l37x29_far_cplx"):
        a, b = xc.device_sums(emu_lib, name), xc.device_sums(emu_lib, name)
        assert np.array_equal(a.view(np.float64), b.view(np.float64)), name


def _raw_call(lib, c, n_u=None, n_pts=None, null=(), out=None):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)           # noqa: E731
    cur = np.ascontiguousarray(c["cur"])
    args = [c["u"], c["v"], c["wu"], c["wv"], cur]
    ptr = [None if i in null else p(a) for i, a in enumerate(args)]
    pts = [None if 5 + i in null else p(a) for i, a in enumerate((c["pu"], c["pv"], c["pw"]))]
    return lib.dll.fdtd_near_field(0, len(c["u"]) if n_u is None else n_u, len(c["v"]), *ptr, c["w0"], c["k"].real, c["k"].imag,
                                   len(c["pu"]) if n_pts is None else n_pts, *pts, None if 8 in null else p(out))


def test_no_points_and_bad_arguments(emu_lib):
    c = xc.case("l37x29_near_real")
    out = np.full((len(c["pu"]), 12), 7.0 + 3.0j)
    assert _raw_call(emu_lib, c, n_pts=0, out=out) == 0 and (out == 7.0 + 3.0j).all()          # returns without touching out
    assert emu_lib.near_field(c["u"], c["v"], c["wu"], c["wv"], c["cur"], c["w0"], c["k"], [], [], []).shape == (0, 12)
    for null in ((0,), (4,), (6,), (8,)):
        assert _raw_call(emu_lib, c, null=null, out=out) < 0 and "fdtd_near_field: bad argument" in emu_lib.error(None), null
    assert _raw_call(emu_lib, c, n_u=0, out=out) < 0 and "bad argument" in emu_lib.error(None)
    assert _raw_call(emu_lib, c, n_pts=-1, out=out) < 0
    assert (out == 7.0 + 3.0j).all()
    with pytest.raises(SolverLibraryError, match="fdtd_near_field_chunks"):
        emu_lib.near_field_chunks(1, 0, 4)


def test_a_point_on_a_node_is_not_finite(emu_lib):
    c = xc.case("l37x29_near_real")
    got = emu_lib.near_field(c["u"], c["v"], c["wu"], c["wv"], c["cur"], c["w0"], c["k"], [c["u"][3], 0.01], [c["v"][5], 0.02],
                             [c["w0"], c["w0"] + 0.4])
    assert not np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(emu_lib):
    disc = discretize(xc.simulation(), n_steps=xc.N_STEPS)
    raw, _ = run_engine(disc.spec, emu_lib)
    sd = {mode: assemble(disc, raw, device_lib=emu_lib, exact_projection_device=mode) for mode in (True, False, None)}
    return dict(disc=disc, raw=raw, sd=sd, ref=xc.end_to_end_reference(disc, raw))


def test_end_to_end_device_against_host(ctx):
    dev, host = ctx["sd"][True], ctx["sd"][False]
    xc.same_containers(dev, host)
    floor, f_at = xc.end_deviation(host, ctx["ref"])
    d, at = xc.end_deviation(dev, ctx["ref"])
    print(f"[exact projection] emulator end to end: floor {floor:.3e} {f_at}, deviation {d:.3e} {at}, ratio {d / floor:.3f} (bar {xc.FACTOR})")
    assert floor > 0 and d <= xc.FACTOR * floor, (d, floor, at)
    assert {n: p for n, (p, _) in xc.log_paths(dev).items()} == {"box": "device", "lossy": "device"}
    assert {n: p for n, (p, _) in xc.log_paths(host).items()} == {"box": "host", "lossy": "host"}


def test_selection_by_work(ctx, emu_lib, monkeypatch):
    auto = ctx["sd"][None]
    paths = xc.log_paths(auto)
    assert {n: p for n, (p, _) in paths.items()} == {"box": "host", "lossy": "host"}
    # pairs = sum over surfaces of n_points x n_u x n_v x n_freq
    for plan in ctx["disc"].plans:
        n_pts = len(xc.observation_points(plan.monitor)[0])
        assert paths[plan.monitor.name][1] == projection.exact_pairs(ctx["disc"], plan, n_pts) < projection.EXACT_HOST_PAIRS
    xc.same_values(auto, ctx["sd"][False])                       # below the threshold: the host path, bit for bit
    assert projection.EXACT_HOST_PAIRS == 1 << 22
    monkeypatch.setattr(projection, "EXACT_HOST_PAIRS", 1)
    forced = assemble(ctx["disc"], ctx["raw"], device_lib=emu_lib, exact_projection_device=None)
    assert {n: p for n, (p, _) in xc.log_paths(forced).items()} == {"box": "device", "lossy": "device"}
    xc.same_values(forced, ctx["sd"][True])
    no_lib = assemble(ctx["disc"], ctx["raw"], exact_projection_device=None)               # nothing to run it on: host
    assert {n: p for n, (p, _) in xc.log_paths(no_lib).items()} == {"box": "host", "lossy": "host"}


def test_device_path_without_a_library_raises(ctx):
    with pytest.raises(SolverLibraryError, match="exact_projection_device=True"):
        assemble(ctx["disc"], ctx["raw"], exact_projection_device=True)


def test_web_run_takes_the_keyword(ctx, emu_lib):
    sd = web.run(xc.simulation(), lib=emu_lib, n_steps=xc.N_STEPS, verbose=False, exact_projection_device=True)
    assert {n: p for n, (p, _) in xc.log_paths(sd).items()} == {"box": "device", "lossy": "device"}
    xc.same_values(sd, ctx["sd"][True])
    assert "Solver time" in sd.log                             # the lines of the run are still there
