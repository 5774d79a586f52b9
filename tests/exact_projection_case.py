"""The cases shared by tests/test_emu_exact_projection.py (emulator) and tests/test_gpu_exact_projection.py (device), their
reference and their bar: the surface integrals of the exact projection (far_field_approx=False) on the device (``fdtd_near_field``,
kernel K9b, csrc/fdtd_near_field.hpp) against the host path (``projection._exact_fields``).

Reference and bar (the rule of docs/history/DENSE_STATE.md).  ``twelve_sums`` is the text of ``projection._exact_fields`` in the
surface's local frame; evaluated in np.longdouble / np.clongdouble it is the reference, evaluated in float64 / complex128 it is the
host path's own arithmetic.  The FLOOR of a case is the worst deviation of the float64 evaluation from the reference over the
case's points and the twelve sums, relative to the largest reference magnitude among the sums of the same kind (I_J, I_M, C_J, C_M)
in the case.  The device and the emulator are held to BAR = 8 x the floor of the same case, by the same measure: nothing absolute
is added.  Cases with many points take the reference (and floor and bar) on ``ref_idx``, a few points spread over the set.

Kernel-level cases: synthetic dense random currents, wavelength 1 (lattice step 0.1), no time stepping.  End-to-end: one small
simulation with a closed box monitor (six surfaces: every axis, both signs; two frequencies) and a windowed surface monitor in a
lossy projection medium; the six spherical components by the same measure, relative to the largest component of the monitor and
frequency (E components over the three E, H over the three H), floor = the host path against a longdouble evaluation of the same
integrals from the same currents."""
import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import projection
from tidy3d_amd.constants import EPSILON_0, MU_0

FACTOR = 8                        # DENSE_STATE's
KINDS = ("I_J", "I_M", "C_J", "C_M")
K0 = 2 * np.pi                    # wavelength 1


def _lattice(n_u, n_v, step=0.1):
    u = (np.arange(n_u) - 0.5 * (n_u - 1)) * step if n_u > 1 else np.array([0.07])
    v = (np.arange(n_v) - 0.5 * (n_v - 1)) * step if n_v > 1 else np.array([-0.03])
    return u, v


def _points(where, n, u, v, w0, rng):
    """n points: 0.3 wavelengths above the plane, at 50 wavelengths, or at 3000 wavelengths off axis"""
    hu, hv = max(0.5 * (u[-1] - u[0]), 0.2), max(0.5 * (v[-1] - v[0]), 0.2)
    if where == "near":
        return rng.uniform(-hu, hu, n), rng.uniform(-hv, hv, n), np.full(n, w0 + 0.3)
    if where == "mid":
        return rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), w0 + 50.0 + rng.uniform(-1, 1, n)
    th, ph = rng.uniform(0.3, 1.2, n), rng.uniform(0, 2 * np.pi, n)
    return 3000.0 * np.sin(th) * np.cos(ph), 3000.0 * np.sin(th) * np.sin(ph), 3000.0 * np.cos(th)


# name: (n_u, n_v, n_pts, k, where, number of reference points (0: all))
CASES = {
    "l37x29_near_real": (37, 29, 7, K0, "near", 0),
    "l37x29_mid_cplx": (37, 29, 7, K0 * (1 + 0.002j), "mid", 0),
    "l37x29_far_real": (37, 29, 7, K0, "far", 0),                        # k R = 1.9e4 rad
    "l37x29_far_cplx": (37, 29, 7, K0 * (1 + 1e-4j), "far", 0),
    "l37x29_one_point": (37, 29, 1, K0 * (1 + 0.01j), "near", 0),
    "line1x40_near": (1, 40, 5, K0, "near", 0),                          # n_u == 1: weight 1
    "l2x2_mid_cplx": (2, 2, 5, K0 * (1 + 0.002j), "mid", 0),
    # either side of the chunk rule's thresholds in n_pts: 2 | 1 chunks of the 1073 nodes, 9 | 5 chunks of the 8281
    "l37x29_p1023": (37, 29, 1023, K0, "mid", 8),
    "l37x29_p1024": (37, 29, 1024, K0, "mid", 8),
    "l91x91_p127": (91, 91, 127, K0 * (1 + 0.002j), "near", 8),
    "l91x91_p128": (91, 91, 128, K0 * (1 + 0.002j), "near", 8),
}
CHUNKS = {"l37x29_near_real": 2, "l37x29_one_point": 2, "line1x40_near": 1, "l2x2_mid_cplx": 1,
          "l37x29_p1023": 2, "l37x29_p1024": 1, "l91x91_p127": 9, "l91x91_p128": 5}
MID_SIZE = ("l96x96_p4096", (96, 96, 64 * 64, K0 * (1 + 0.002j), "plane", 16))      # device only: 3.8e7 pairs
_cache = {}


def case(name):
    """dict of the case's inputs (float64 / complex128, as the library takes them), built once"""
    if name in _cache:
        return _cache[name]
    n_u, n_v, n_pts, k, where, n_ref = CASES[name] if name in CASES else MID_SIZE[1]
    rng = np.random.default_rng(sum(map(ord, name)))
    u, v = _lattice(n_u, n_v)
    w0 = 0.25
    cur = rng.standard_normal((4, n_u, n_v)) + 1j * rng.standard_normal((4, n_u, n_v))
    if where == "plane":                 # a focal-plane grid 5 wavelengths above the surface
        g = np.linspace(-4.0, 4.0, 64)
        pu, pv = (a.ravel() for a in np.meshgrid(g, g + 0.013, indexing="ij"))
        pw = np.full(pu.size, w0 + 5.0)
    else:
        pu, pv, pw = _points(where, n_pts, u, v, w0, rng)
    idx = np.arange(n_pts) if not n_ref else np.unique(np.linspace(0, n_pts - 1, n_ref).round().astype(int))
    c = dict(name=name, u=u, v=v, wu=projection._trap_weights(u), wv=projection._trap_weights(v), cur=cur, w0=w0, k=complex(k),
             pu=pu, pv=pv, pw=pw, ref_idx=idx)
    _cache[name] = c
    return c


def twelve_sums(u, v, w0, cur, k, pu, pv, pw, real=np.float64):
    """[n, 12] I_J, I_M, C_J, C_M (u, v, w components each): the statements of projection._exact_fields in the local frame
    (u, v, w) taken as right-handed, in the arithmetic of ``real`` (np.float64: the host path's; np.longdouble: the reference)"""
    cplx = np.complex128 if real is np.float64 else np.clongdouble
    u, v = np.asarray(u, real), np.asarray(v, real)
    k = cplx(real(np.real(k)) + 1j * real(np.imag(k))) if real is not np.float64 else complex(k)
    src = np.zeros((len(u), len(v), 3), real)
    src[..., 0], src[..., 1], src[..., 2] = u[:, None], v[None, :], real(w0)
    zero = np.zeros((len(u), len(v)), cplx)
    Jc = [cur[0].astype(cplx), cur[1].astype(cplx), zero]
    Mc = [cur[2].astype(cplx), cur[3].astype(cplx), zero]
    four_pi = 4 * (np.pi if real is np.float64 else np.arctan(real(1)) * 4)
    out = np.zeros((len(pu), 12), cplx)
    for n in range(len(pu)):
        pt = np.array([pu[n], pv[n], pw[n]], real)
        Rv = pt[None, None, :] - src
        R = np.sqrt(np.sum(Rv ** 2, axis=-1))
        Rh = [Rv[..., a] / R for a in range(3)]
        G = np.exp(1j * k * R) / (four_pi * R)
        G1 = G * (1j * k - 1.0 / R)
        G2 = G1 * (1j * k - 1.0 / R) + G / R ** 2
        for f, c in enumerate((Jc, Mc)):
            rd = Rh[0] * c[0] + Rh[1] * c[1] + Rh[2] * c[2]
            cx = [Rh[1] * c[2] - Rh[2] * c[1], Rh[2] * c[0] - Rh[0] * c[2], Rh[0] * c[1] - Rh[1] * c[0]]
            for a in range(3):
                pot = G * c[a] + (Rh[a] * rd * G2 + (c[a] - Rh[a] * rd) * G1 / R) / k ** 2
                out[n, 3 * f + a] = projection._trapz2(pot, u, v)
                out[n, 6 + 3 * f + a] = projection._trapz2(G1 * cx[a], u, v)
    return out


def deviation(got, ref):
    """worst |got - ref| over points and sums, relative to the largest |ref| among the sums of the same kind; and the kind"""
    worst, at = 0.0, None
    for i, kind in enumerate(KINDS):
        r = ref[:, 3 * i:3 * i + 3]
        scale = float(np.abs(r).max())
        assert scale > 0, kind
        d = float(np.abs(got[:, 3 * i:3 * i + 3].astype(np.clongdouble) - r).max()) / scale
        if d >= worst:
            worst, at = d, kind
    return worst, at


def reference(name):
    """(reference [len(ref_idx), 12] clongdouble, floor) of the case, computed once and left unchanged"""
    key = ("ref", name)
    if key not in _cache:
        c = case(name)
        i = c["ref_idx"]
        args = (c["u"], c["v"], c["w0"], c["cur"], c["k"], c["pu"][i], c["pv"][i], c["pw"][i])
        ref = twelve_sums(*args, real=np.longdouble)
        floor, _ = deviation(twelve_sums(*args, real=np.float64), ref)
        ref.setflags(write=False)
        _cache[key] = (ref, floor)
    return _cache[key]


def device_sums(lib, name):
    c = case(name)
    return lib.near_field(c["u"], c["v"], c["wu"], c["wv"], c["cur"], c["w0"], c["k"], c["pu"], c["pv"], c["pw"])


def check_case(lib, name, label):
    """the device's (or the emulator's) twelve sums of the case within FACTOR x floor of the reference; prints the figures"""
    ref, floor = reference(name)
    got = device_sums(lib, name)
    assert got.shape == (len(case(name)["pu"]), 12) and got.dtype == np.complex128
    dev, at = deviation(got[case(name)["ref_idx"]], ref)
    print(f"[exact projection] {label} {name}: floor {floor:.3e}, deviation {dev:.3e} ({at}), ratio {dev / floor:.3f} (bar {FACTOR})")
    assert floor > 0, name
    assert dev <= FACTOR * floor, (name, dev, floor, at)
    return got


# ---- end to end ----------------------------------------------------------------------------------------------------------------

N_STEPS = 60
FREQS = (2.6e14, 3.3e14)
SPHERICAL = ("Er", "Etheta", "Ephi", "Hr", "Htheta", "Hphi")
E2E_NAMES = ("box", "lossy")


def simulation():
    f0 = 3e14
    pulse = td.GaussianPulse(freq0=f0, fwidth=f0 / 5)
    return td.Simulation(
        size=(2.2, 2.2, 2.2), grid_spec=td.GridSpec.uniform(dl=0.1), run_time=30 / f0,
        sources=[td.PointDipole(center=(0, 0, 0), source_time=pulse, polarization="Ex"),
                 td.PointDipole(center=(0.1, -0.1, 0.05), source_time=pulse, polarization="Ez")],
        monitors=[td.FieldProjectionAngleMonitor(center=(0.02, 0, -0.03), size=(1.0, 1.1, 0.9), freqs=FREQS, theta=(0.5, 1.4, 2.5),
                                                 phi=(0.2, 2.9), proj_distance=40.0, far_field_approx=False, name="box"),
                  td.FieldProjectionCartesianMonitor(center=(0, 0, 0.5), size=(1.6, 1.4, 0), freqs=FREQS[:1], normal_dir="+",
                                                     x=(-0.7, 0.4), y=(0.3, 1.1), proj_distance=3.0, proj_axis=2,
                                                     window_size=(0.3, 0.2), far_field_approx=False, name="lossy",
                                                     medium=td.Medium(permittivity=2.0, conductivity=0.02))],
        boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=6)), shutoff=0)


def observation_points(mon):
    """([n, 3] points relative to the local origin, theta, phi) as project_angle / project_cartesian form them"""
    if not isinstance(mon, td.FieldProjectionCartesianMonitor):
        T, P = np.meshgrid(np.asarray(mon.theta, float), np.asarray(mon.phi, float), indexing="ij")
        t, p = T.ravel(), P.ravel()
        return float(mon.proj_distance) * np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], axis=1), t, p
    loc = [np.atleast_1d(np.asarray(mon.x, float)), np.atleast_1d(np.asarray(mon.y, float))]
    loc.insert(int(mon.proj_axis), np.atleast_1d(float(mon.proj_distance)))
    X, Y, Z = np.meshgrid(*loc, indexing="ij")
    r = np.sqrt(X ** 2 + Y ** 2 + Z ** 2).ravel()
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), np.arccos(Z.ravel() / r), np.arctan2(Y.ravel(), X.ravel())


def end_to_end_reference(disc, raw):
    """name -> {component: clongdouble [n_points, n_freq]}: the monitor's six spherical components from the host path's own
    currents (projection._surface_currents), the integrals and everything behind them in longdouble"""
    from tidy3d_amd.data import source_spectrum_fn
    norm = source_spectrum_fn(disc, disc.sim.normalize_index)
    ld, cld = np.longdouble, np.clongdouble
    pi = np.arctan(ld(1)) * 4
    out = {}
    for plan in disc.plans:
        mon = plan.monitor
        if mon.name not in E2E_NAMES:
            continue
        freqs = np.asarray(mon.freqs, float)
        medium, eps_f, k_f, _ = projection._medium_params(mon, disc.sim, None, freqs)
        pts_o, th, ph = observation_points(mon)
        origin = np.asarray(mon.local_origin, float)
        E = np.zeros((3, len(pts_o), len(freqs)), cld)
        H = np.zeros_like(E)
        for axis, u, v, pts, J, M in projection._surface_currents(disc, plan, raw, norm, medium):
            hand = -1 if axis == 1 else 1
            for i_f, f in enumerate(freqs):
                cur = np.stack([J[u][:, :, i_f], J[v][:, :, i_f], M[u][:, :, i_f], M[v][:, :, i_f]])
                p = (pts_o + origin).astype(ld)               # the points as both paths take them: formed in float64
                s = twelve_sums(pts[u], pts[v], pts[axis][0], cur, k_f[i_f], p[:, u], p[:, v], p[:, axis], real=ld)
                w = 2 * pi * ld(f)
                ce, ch = 1j * w * ld(MU_0), 1j * w * ld(EPSILON_0) * cld(eps_f[i_f])
                for j, a in enumerate((u, v, axis)):
                    E[a, :, i_f] += ce * s[:, j] - hand * s[:, 9 + j]
                    H[a, :, i_f] += ch * s[:, 3 + j] + hand * s[:, 6 + j]
        st, ct, sp, cp = (fn(x.astype(ld))[:, None] for fn, x in ((np.sin, th), (np.cos, th), (np.sin, ph), (np.cos, ph)))
        comps = {}
        for g, F in (("E", E), ("H", H)):
            comps[g + "r"] = F[0] * st * cp + F[1] * st * sp + F[2] * ct
            comps[g + "theta"] = F[0] * ct * cp + F[1] * ct * sp - F[2] * st
            comps[g + "phi"] = -F[0] * sp + F[1] * cp
        out[mon.name] = comps
    return out


def end_deviation(sd, ref):
    """worst over monitors, components and frequencies of |value - reference| / S, S = the largest |reference component| of the
    monitor and frequency (over the three E components for an E component, the three H for an H component); and where"""
    worst, at = 0.0, None
    for n in E2E_NAMES:
        nf = ref[n]["Er"].shape[-1]
        for g in "EH":
            scale = np.max([np.abs(ref[n][c]).max(axis=0) for c in SPHERICAL if c[0] == g], axis=0)
            assert (scale > 0).all(), (n, g)
            for c in (c for c in SPHERICAL if c[0] == g):
                val = np.asarray(getattr(sd[n], c).values).reshape(-1, nf).astype(np.clongdouble)
                r = float(np.max(np.abs(val - ref[n][c]).max(axis=0) / scale))
                if r >= worst:
                    worst, at = r, (n, c)
    return worst, at


def same_containers(a, b):
    for n in E2E_NAMES:
        assert type(a[n]) is type(b[n]), n
        for c in SPHERICAL:
            xa, xb = getattr(a[n], c), getattr(b[n], c)
            assert np.asarray(xa.values).dtype == np.asarray(xb.values).dtype and xa.dims == xb.dims and list(xa.coords) == list(xb.coords), (n, c)
            assert np.asarray(xa.values).shape == np.asarray(xb.values).shape, (n, c)
            assert all(np.array_equal(np.asarray(xa.coords[k]), np.asarray(xb.coords[k])) for k in xa.coords), (n, c)


def same_values(a, b):
    for n in E2E_NAMES:
        for c in SPHERICAL:
            x, y = np.asarray(getattr(a[n], c).values), np.asarray(getattr(b[n], c).values)
            assert np.array_equal(x.view(np.float64), y.view(np.float64)), (n, c)


def log_paths(sd):
    """monitor name -> (path, pairs) from the lines data.assemble writes into SimulationData.log"""
    import re
    return {m.group(1): (m.group(2), int(m.group(3)))
            for m in re.finditer(r"Exact projection of monitor '([^']+)': (device|host), (\d+) point-node pairs", sd.log or "")}
