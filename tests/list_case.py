"""What the tests of the whole-grid node lists share (tests/modulation_case.py, tests/nonlinear_case.py, tests/pec_conformal_case.py and
their test_emu_* / test_gpu_* files): the scenario with its state and cached fp64 references, the comparison with the emulator's
committed record, the off-reason check and the lifecycle skeleton.  A kind keeps what is its own — oracle subclass, media, scenarios,
bars — and names it on its ``Scenario`` subclass."""
import dataclasses
import os

import numpy as np

from tidy3d_amd import lib as L
from tidy3d_amd.engine import HipEngine
from oracle.fdtd_numpy import OracleFdtd

import dense_state as ds

PATHS = ("fused", "twopass")
ULPS = 4
_CACHE = {}


def golden(kind):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", kind, "emulator_k7.npz")


class Scenario:
    """A spec with its state and its fp64 references (with and without the lists), computed once per process and never changed.
    A subclass sets ATTR (the lists' attribute on the spec), TAG (of the printed lines), ORACLE, SCENARIOS (label -> spec), BAR, GOLDEN."""
    ATTR = TAG = ORACLE = SCENARIOS = BAR = GOLDEN = None

    def __init__(self, label):
        self.label, self.spec = label, self.SCENARIOS[label]()
        assert self.lists, label
        self.plain = dataclasses.replace(self.spec, **{self.ATTR: []})
        self.state, _ = ds.admissible_state(self.plain, seed=1)
        self._ref, self._plain = {}, {}

    @property
    def lists(self):
        return getattr(self.spec, self.ATTR)

    def _run(self, cls, spec, K):
        o = cls(spec)
        ds._load(o, self.state)
        for _ in range(K):
            o.step()
        return [np.array(f) for f in o.E + o.H]

    def ref_spec(self):
        return self.spec

    def ref(self, K, *how):
        """the fields of the kind's fp64 oracle after K steps (``how``: what ``ref_spec`` takes)"""
        if (K, *how) not in self._ref:
            self._ref[(K, *how)] = self._run(self.ORACLE, self.ref_spec(*how), K)
        return self._ref[(K, *how)]

    def ref_plain(self, K):
        if K not in self._plain:
            self._plain[K] = self._run(OracleFdtd, self.plain, K)
        return self._plain[K]

    def listed_diff(self, a, b):
        """rel-L2 between two field sets over the listed nodes (all listed components together)"""
        num = den = 0.0
        for s in self.lists:
            i = (s.ijk[:, 2], s.ijk[:, 1], s.ijk[:, 0])
            num += float(np.sum(np.abs(a[s.comp][i] - b[s.comp][i]) ** 2))
            den += float(np.sum(np.abs(a[s.comp][i]) ** 2))
        return float(np.sqrt(num / den))

    def visibility(self, K):
        """rel-L2 between the fp64 references with and without the lists over the listed nodes"""
        return self.listed_diff(self.ref(K), self.ref_plain(K))

    def errors(self, fields, K, *how):
        """per field |got - ref| / |ref| (L2 over the whole array) against the kind's fp64 oracle"""
        ref = self.ref(K, *how)
        return [float(np.linalg.norm(np.asarray(fields[c], np.result_type(fields[c], np.float64)) - ref[c]) / np.linalg.norm(ref[c]))
                for c in range(6)]

    def run(self, lib, K, path, plain=False, **kw):
        return ds.run_engine(self.plain if plain else self.spec, lib, self.state, K, path, **kw)

    def listed_values(self, fields):
        """the fields at the listed nodes, list after list: what the emulator's record holds (fp32 parts)"""
        v = np.concatenate([np.asarray(fields[s.comp])[s.ijk[:, 2], s.ijk[:, 1], s.ijk[:, 0]] for s in self.lists])
        return v.astype(np.complex64 if np.iscomplexobj(v) else np.float32)


def scenario(cls, label):
    if (cls, label) not in _CACHE:
        _CACHE[cls, label] = cls(label)
    return _CACHE[cls, label]


def emulator_record(cls, lib):
    """label -> listed_values of the fused run of 7 steps (the kind's test_emu_* file holds the committed file to the emulator's bits)"""
    return {label: scenario(cls, label).listed_values(scenario(cls, label).run(lib, 7, "fused").fields) for label in cls.SCENARIOS}


def check_against_emulator_record(sc, fields):
    """the device within ULPS fp32 ulps of the largest listed value of the emulator's run; -> (largest difference in those ulps, equal bits?)"""
    want = np.load(sc.GOLDEN)[sc.label]
    got = sc.listed_values(fields)
    assert got.shape == want.shape and got.dtype == want.dtype
    ulp = float(np.spacing(np.float32(max(np.abs(want.real).max(), np.abs(want.imag).max()))))
    diff = got.astype(np.complex128) - want.astype(np.complex128)
    worst = float(max(np.abs(diff.real).max(), np.abs(diff.imag).max())) / ulp
    print(f"[{sc.TAG}] {sc.label}: device against the emulator's record: {worst:.2f} ulp of the largest value, equal bits: {np.array_equal(got, want)}")
    assert worst <= ULPS, (sc.label, worst)
    return worst, bool(np.array_equal(got, want))


def off_reason(lib, spec, plain, reason, name):
    """128 x 128 x 64, 4 steps: no pairs under ``reason``, which the library's table calls ``name``; ``plain`` — the same grid without
    the lists — does take pairs"""
    assert spec.shape == plain.shape == (128, 128, 64) and L.F2_OFF_REASONS[reason] == name
    with HipEngine(spec, lib=lib) as e:
        st = e.run(4)
    assert int(st.fused2_pairs) == 0 and int(st.fused2_off_reason) == reason, (int(st.fused2_pairs), int(st.fused2_off_reason))
    with HipEngine(plain, lib=lib) as e:
        assert int(e.run(4).fused2_pairs) == 2


def lifecycle(lib, sc, variant, twostep_off=True, mid=True, steps=None, **kw):
    """run(7) == fdtd_reset + run(7) == fdtd_reset + run(3) + run(4), under the kind's bar; with ``mid``, a set_field in mid-run is held
    to a fresh handle that took its first three steps from that other state (the step count is part of the state; not for a scenario
    with CPML or dispersive bodies, whose states a set_field does not replace).  ``steps(engine, load, fields, whole)``: the kind's own.
    -> the fields of run(7)"""
    state2 = ds.admissible_state(sc.plain, seed=2)[0] if mid else None

    def engine(spec=sc.spec):
        e = HipEngine(spec, lib=lib, variant=variant, **kw)
        if twostep_off:
            e.set_option(L.OPT_TWOSTEP, 0)
        return e

    def fields(e):
        return [e.get_field(c) for c in range(6)]

    def load(e, state=sc.state):
        for c in range(6):
            e.set_field(c, state[c])

    def run(e, *parts, reset=True):
        """(from a reset,) per (state or None, steps): a set_field of all six fields, a run"""
        if reset:
            e.reset()
        for state, n in parts:
            if state is not None:
                load(e, state)
            e.run(n)
        return fields(e)
    with engine() as e:
        whole = run(e, (sc.state, 7), reset=False)
        again = run(e, (sc.state, 7))
        split = run(e, (sc.state, 3), (None, 4))
        changed = run(e, (sc.state, 3), (state2, 4)) if mid else None
    if mid:
        with engine() as e:
            fresh = run(e, (state2, 3), (state2, 4), reset=False)
    for c in range(6):
        assert np.array_equal(whole[c], again[c]) and np.array_equal(whole[c], split[c]), ds.COMP[c]
        if mid:
            assert np.array_equal(changed[c], fresh[c]) and not np.array_equal(changed[c], whole[c]), ds.COMP[c]
    assert max(sc.errors(whole, 7)) <= sc.BAR
    if steps:
        steps(engine, load, fields, whole)
    return whole
