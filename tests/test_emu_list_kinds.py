"""The four kinds of whole-grid node lists — fully anisotropic coupling, time-modulated media, PEC-conformal faces, Kerr media — at
the C entry points, on the emulator: every site that refuses a kind, with the error string written out; the index checks of every
fdtd_add_*; which kind the step-pair off-reason names when a handle holds two.  An 8 x 8 x 8 PEC box, lists of one node; every
refusal comes before any launch, the off-reason runs take two steps each.

The row of each kind (csrc/fdtd_capi.hip, the table beside the group structs) is what these strings spell out:
  fully anisotropic media    accepted by fdtd_add_aniso and fdtd_comm_init on z-slabs, refused by fdtd_run / fdtd_run_bloch there;
                             a Bloch pair carries the same lists on both handles
  time-modulated media       refused on z-slabs by fdtd_add_modulation and fdtd_comm_init; the same lists on both handles
  PEC-conformal boundaries   refused on z-slabs by fdtd_add_pec_conformal and fdtd_comm_init; the same lists on both handles
  nonlinear media            refused on z-slabs by fdtd_add_nonlinear and fdtd_comm_init; refused by fdtd_run_bloch
(fdtd_run and fdtd_run_bloch name the last three on z-slabs as well, but no sequence of calls reaches those lines: a handle
cannot hold such a list and a communicator at once.)"""
import ctypes as C

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine, _f32, _ptr

import modulation_case as mc

N = 8
NCELL = N * N * N
NODE = (3 * N + 3) * N + 3          # cell (3, 3, 3)
NONE = 0xFFFFFFFF
W5 = 5 + 64 * 3                     # FDTD_OPT_TWOSTEP: five waves x three planes — a shape this grid can hold, so the lists decide
KINDS = ("aniso", "modulation", "conformal", "nonlinear")
WHO = {"aniso": "fdtd_add_aniso", "modulation": "fdtd_add_modulation", "conformal": "fdtd_add_pec_conformal", "nonlinear": "fdtd_add_nonlinear"}
NOUN = {"aniso": "fully anisotropic media", "modulation": "time-modulated media", "conformal": "PEC-conformal boundaries",
        "nonlinear": "nonlinear media"}


@pytest.fixture(scope="module")
def spec():
    pec = td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec())
    s = discretize(mc._box_sim((N, N, N), pec, sources=()), n_steps=1).spec
    s.decay_every = 0
    assert s.shape == (N, N, N)
    return s


def u32(*v):
    return np.ascontiguousarray(np.asarray(v, np.uint32))


def add(lib, h, kind, cell=NODE, nbr=NONE, bloch=False):
    """one list of one node of ``kind`` on handle ``h`` (component x: 0, or 3 for the conformal faces) -> the call's status"""
    d, c = lib.dll, u32(cell)
    one, zero = _f32([1.0]), _f32([0.0])
    if kind == "aniso":
        n8, w = u32(*[nbr] * 8), _f32([0.0] * 8)
        if bloch:
            return d.fdtd_add_aniso_bloch(h, 0, 1, _ptr(c), _ptr(n8), _ptr(w), _ptr(w), _ptr(np.zeros(8, np.uint8)))
        return d.fdtd_add_aniso(h, 0, 1, _ptr(c), _ptr(n8), _ptr(w), _ptr(w))
    if kind == "modulation":
        z2 = _f32([0.0, 0.0])
        return d.fdtd_add_modulation(h, 0, 1, _ptr(c), _ptr(one), _ptr(one), _ptr(zero), _ptr(z2), _ptr(z2), 0.1, 0.0)
    if kind == "conformal":
        return d.fdtd_add_pec_conformal(h, 3, 1, _ptr(c), _ptr(u32(*[nbr] * 4)), _ptr(_f32([0.0] * 4)))
    return d.fdtd_add_nonlinear(h, 0, 1, _ptr(c), _ptr(u32(*[nbr] * 8)), _ptr(one), _ptr(one), _ptr(zero), _ptr(zero), 5)


def refused(lib, h, status, message):
    assert status < 0 and lib.error(h) == message, (status, lib.error(h))


def run(lib, h):
    return lib.dll.fdtd_run(h, 1, C.cast(None, L.PROGRESS_FN), None)


def run_bloch(lib, hr, hi):
    return lib.dll.fdtd_run_bloch(hr, hi, 1, (C.c_double * 3)(0.7, 0.0, 0.0), (C.c_int * 3)(0, 0, 0), C.cast(None, L.PROGRESS_FN), None)


def with_comm(spec, lib):
    """a handle for a communicator of one rank (the emulator's RCCL shim): PEC z faces, fdtd_comm_init not yet called"""
    return HipEngine(spec, lib=lib, force_comm=True)


# ---------------------------------------------------------------------------------------------------------------- z-slabs
@pytest.mark.parametrize("kind", KINDS)
def test_add_on_a_handle_with_a_neighbour_face(kind, spec, emu_lib):
    with HipEngine(spec, lib=emu_lib, slab=(0, 4), rank=0, n_ranks=2) as e:          # (its upper z face is FDTD_BC_NEIGHBOR)
        st = add(emu_lib, e.handle, kind)
        if kind == "aniso":
            assert st == 0
        else:
            refused(emu_lib, e.handle, st, f"{WHO[kind]}: {NOUN[kind]} are not available on z-slabs")


@pytest.mark.parametrize("kind", KINDS)
def test_add_on_a_handle_with_a_communicator(kind, spec, emu_lib):
    with with_comm(spec, emu_lib) as e:
        e.comm_init(e.unique_id())
        st = add(emu_lib, e.handle, kind)
        if kind == "aniso":
            assert st == 0
        else:
            refused(emu_lib, e.handle, st, f"{WHO[kind]}: {NOUN[kind]} are not available on z-slabs")


@pytest.mark.parametrize("kind", KINDS)
def test_comm_init_and_run_on_a_handle_that_holds_lists(kind, spec, emu_lib):
    with with_comm(spec, emu_lib) as e:
        assert add(emu_lib, e.handle, kind) == 0
        st = emu_lib.dll.fdtd_comm_init(e.handle, C.create_string_buffer(e.unique_id(), 128), 0, 1)
        if kind != "aniso":
            refused(emu_lib, e.handle, st, f"fdtd_comm_init: {NOUN[kind]} are not available on z-slabs")
            return
        assert st == 0                      # the row's exception: fully anisotropic lists are refused by the run only
        refused(emu_lib, e.handle, run(emu_lib, e.handle), "fdtd_run: fully anisotropic media are not available on z-slabs")


def test_run_bloch_refuses_anisotropic_lists_on_z_slabs(spec, emu_lib):
    with with_comm(spec, emu_lib) as er, HipEngine(spec, lib=emu_lib) as ei:
        er.comm_init(er.unique_id())
        for e in (er, ei):
            assert add(emu_lib, e.handle, "aniso", bloch=True) == 0
        refused(emu_lib, er.handle, run_bloch(emu_lib, er.handle, ei.handle),
                "fdtd_run_bloch: fully anisotropic media are not available on z-slabs")


# ---------------------------------------------------------------------------------------------------------------- Bloch pairs
BLOCH = {"aniso": "fdtd_run_bloch: the two solvers must carry the same fully anisotropic lists",
         "modulation": "fdtd_run_bloch: the two solvers must carry the same time-modulation lists",
         "conformal": "fdtd_run_bloch: the two solvers must carry the same PEC-conformal lists",
         "nonlinear": "fdtd_run_bloch: nonlinear media are not available with Bloch boundaries"}


@pytest.mark.parametrize("on", ["first", "second"])
@pytest.mark.parametrize("kind", KINDS)
def test_run_bloch_with_unequal_lists(kind, on, spec, emu_lib):
    with HipEngine(spec, lib=emu_lib) as er, HipEngine(spec, lib=emu_lib) as ei:
        assert add(emu_lib, (er if on == "first" else ei).handle, kind) == 0
        refused(emu_lib, er.handle, run_bloch(emu_lib, er.handle, ei.handle), BLOCH[kind])


def test_run_bloch_with_nonlinear_lists_on_both_handles(spec, emu_lib):
    with HipEngine(spec, lib=emu_lib) as er, HipEngine(spec, lib=emu_lib) as ei:
        for e in (er, ei):
            assert add(emu_lib, e.handle, "nonlinear") == 0
        refused(emu_lib, er.handle, run_bloch(emu_lib, er.handle, ei.handle), BLOCH["nonlinear"])


def test_run_bloch_compares_component_and_length(spec, emu_lib):
    with HipEngine(spec, lib=emu_lib) as er, HipEngine(spec, lib=emu_lib) as ei:
        d, c, z4 = emu_lib.dll, u32(NODE), _f32([0.0] * 4)
        assert d.fdtd_add_pec_conformal(er.handle, 3, 1, _ptr(c), _ptr(u32(*[NONE] * 4)), _ptr(z4)) == 0
        assert d.fdtd_add_pec_conformal(ei.handle, 4, 1, _ptr(c), _ptr(u32(*[NONE] * 4)), _ptr(z4)) == 0
        refused(emu_lib, er.handle, run_bloch(emu_lib, er.handle, ei.handle), BLOCH["conformal"])


# ---------------------------------------------------------------------------------------------------------------- indices
@pytest.mark.parametrize("kind", KINDS)
def test_index_checks(kind, spec, emu_lib):
    with HipEngine(spec, lib=emu_lib) as e:
        refused(emu_lib, e.handle, add(emu_lib, e.handle, kind, cell=NCELL), f"{WHO[kind]}: cell index out of range")
        if kind != "modulation":            # (the modulation lists carry no neighbour slots)
            refused(emu_lib, e.handle, add(emu_lib, e.handle, kind, nbr=NCELL), f"{WHO[kind]}: neighbour index out of range")
        if kind == "aniso":
            refused(emu_lib, e.handle, add(emu_lib, e.handle, kind, cell=NCELL, bloch=True), "fdtd_add_aniso_bloch: cell index out of range")
            refused(emu_lib, e.handle, add(emu_lib, e.handle, kind, nbr=NCELL, bloch=True), "fdtd_add_aniso_bloch: neighbour index out of range")
        assert add(emu_lib, e.handle, kind, cell=NCELL - 1, nbr=NCELL - 1) == 0         # the last cell is in range


def test_modulation_and_nonlinear_lists_exclude_each_other(spec, emu_lib):
    with HipEngine(spec, lib=emu_lib) as e:
        assert add(emu_lib, e.handle, "modulation") == 0
        refused(emu_lib, e.handle, add(emu_lib, e.handle, "nonlinear"),
                "fdtd_add_nonlinear: nonlinear media are not available together with time-modulated media")
    with HipEngine(spec, lib=emu_lib) as e:
        assert add(emu_lib, e.handle, "nonlinear") == 0
        refused(emu_lib, e.handle, add(emu_lib, e.handle, "modulation"),
                "fdtd_add_modulation: time-modulated media are not available together with nonlinear media")


# ---------------------------------------------------------------------------------------------------------------- off-reason
@pytest.mark.parametrize("kinds,reason", [((), 0), (("aniso",), 5), (("modulation",), 15), (("conformal",), 16), (("nonlinear",), 17),
                                          (("modulation", "aniso"), 5), (("nonlinear", "aniso"), 5), (("conformal", "modulation"), 15),
                                          (("nonlinear", "conformal"), 16)])
def test_off_reason_names_the_first_kind_in_the_tables_order(kinds, reason, spec, emu_lib):
    """(the lists are added in the reverse of the table's order: the order of the calls does not matter)"""
    with HipEngine(spec, lib=emu_lib, axis_shift=0) as e:
        e.set_option(L.OPT_TWOSTEP, W5)
        for kind in kinds:
            assert add(emu_lib, e.handle, kind) == 0
        st = e.run(2)
        assert int(st.fused2_off_reason) == reason and (int(st.fused2_pairs) > 0) == (reason == 0), (int(st.fused2_pairs), int(st.fused2_off_reason))
