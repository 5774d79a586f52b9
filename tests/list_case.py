"""What the tests of the whole-grid node lists share (tests/modulation_case.py, tests/nonlinear_case.py, tests/pec_conformal_case.py and
their test_emu_* / test_gpu_* files): the scenario with its state and cached fp64 references, the comparison with the emulator's
committed record, the off-reason check and the lifecycle skeleton.  A kind keeps what is its own — oracle subclass, media, scenarios,
bars — and names it on its ``Scenario`` subclass.

Node by node (docs/history/LIST_NODES.md): ``Scenario.check_nodes`` holds every node that is not excluded under ds.MARGIN x the floor
of the kind's own fp32 oracle, in the measure of tests/dense_state.py, and says of the worst node whether it is listed, which entry of
which list it is and what its slots hold; ``kerr_slots`` / ``conformal_slots`` build the neighbour slots a second time from the
convention in the kernel headers; the planted deviations change one entry of one list of the reference's spec."""
import dataclasses
import os

import numpy as np

from tidy3d_amd import lib as L
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.spec import BC_PERIODIC
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
    EXTRA = {}                # label -> spec of the small scenarios that are in no committed record (``all_labels``)

    def __init__(self, label):
        self.label, self.spec = label, {**self.SCENARIOS, **self.EXTRA}[label]()
        assert self.lists, label
        self.plain = dataclasses.replace(self.spec, **{self.ATTR: []})
        self.state, self.excluded = ds.admissible_state(self.plain, seed=1)
        self.share = ds.excluded_share(self.excluded)
        self._ref, self._plain, self._floor = {}, {}, {}

    @property
    def lists(self):
        return getattr(self.spec, self.ATTR)

    def _run(self, cls, spec, K, dtype=np.float64):
        o = cls(spec, dtype=dtype)
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

    # ------------------------------------------------------------------------------------------------ node by node
    @classmethod
    def all_labels(cls):
        return list(cls.SCENARIOS) + list(cls.EXTRA)

    def slots_of(self, s):
        """-> (nbr [n, slots, 3], read): the list's own slots, or — a kind whose kernel reads none — the eight nodes around each
        listed node in the Kerr layout, built here"""
        if hasattr(s, "nbr_ijk"):
            return np.asarray(s.nbr_ijk), True
        return kerr_slots(self.spec, s.comp, s.ijk)[1], False

    def wraps_of(self, s, e):
        """what a kind whose lists record the periods crossed adds to the sentence about entry e (tests/aniso_case.py: the signs)"""
        return ""

    def check_inputs(self):
        """what keeps the measure honest: at most SHARE_CAP of the nodes left out, no listed node among them"""
        assert self.share <= SHARE_CAP, f"{self.label}: {100 * self.share:.2f} % of the nodes are excluded"
        for n, s in enumerate(self.lists):
            out = self.excluded[s.comp][s.ijk[:, 2], s.ijk[:, 1], s.ijk[:, 0]]
            assert not out.any(), f"{self.label}: {int(out.sum())} listed nodes of list {n} ({ds.COMP[s.comp]}) are excluded, first {s.ijk[out][0]}"

    def where(self, c, ijk):
        """``ds.where`` and what the lists say of node ``ijk`` = (i, j, k) of component c"""
        ijk = np.asarray(ijk, np.int64)
        out = ds.where(self.spec, c, (ijk[2], ijk[1], ijk[0]))
        for n, s in enumerate(self.lists):
            hit = np.nonzero((s.ijk == ijk[None, :]).all(axis=1))[0] if s.comp == c else ()
            if len(hit):
                e, (nbr, read) = int(hit[0]), self.slots_of(s)
                empty = int((nbr[e, :, 0] < 0).sum())
                wrapped = int(((nbr[e, :, 0] >= 0) & (np.abs(nbr[e] - ijk[None, :]) > 1).any(axis=1)).sum())
                return out + (f"; listed: {self.TAG} list {n} ({ds.COMP[s.comp]}), entry {e} of {len(s.ijk)} (block {e // BLOCK}, lane {e % BLOCK}); "
                              f"{empty} of its {nbr.shape[1]} slots empty, {wrapped} wrapped" + self.wraps_of(s, e) + ("" if read else " (this kind reads no slots)"))
        every = np.concatenate([s.ijk for s in self.lists])
        return out + f"; not listed: {int(np.abs(every - ijk[None, :]).max(axis=1).min())} cells (Chebyshev) from the nearest listed node"

    def measure(self, fields, K, *how, ref=None):
        """-> ds.Worst: the worst node that is not excluded, |got - ref| over the local scale of the fp64 reference (``ds.measure_fields``)"""
        ref = self.ref(K, *how) if ref is None else ref
        w = ds.worst_of(ds.measure_fields(self.spec, self.state, self.excluded, ds.Run(ref, {}), ds.Run([np.asarray(f) for f in fields], {})))
        w.at = self.where(ds.COMP.index(w.comp), w.index)
        return w

    def floor(self, K, *how):
        """the kind's own oracle in fp32 against its fp64 run, in the same measure"""
        if (K, *how) not in self._floor:
            self._floor[(K, *how)] = self.measure(self._run(self.ORACLE, self.ref_spec(*how), K, dtype=np.float32), K, *how)
        return self._floor[(K, *how)]

    def bar_nodes(self, K, *how):
        return ds.MARGIN * self.floor(K, *how).value

    def check_nodes(self, fields, K, what, *how):
        """every node that is not excluded under ds.MARGIN x the floor of (K, how): the bar comes from the reference alone"""
        self.check_inputs()
        w, fl, bar = self.measure(fields, K, *how), self.floor(K, *how), self.bar_nodes(K, *how)
        print(f"[dense] {self.TAG} {self.label} K={K}{''.join(f' {h}' for h in how)} {what}: nodes {w.value:.3e} | floor {fl.value:.3e} bar {bar:.3e} | "
              f"ratio to floor {w.value / max(fl.value, 1e-300):.2f} | excluded {100 * self.share:.2f} % | lists "
              + " ".join(f"{ds.COMP[s.comp]} {len(s.ijk)}" for s in self.lists))
        assert w.value <= bar, f"{self.TAG} {self.label} K={K}{''.join(f' {h}' for h in how)} {what}: node over the bar {bar:.3e} (floor {fl.value:.3e}): {w}"
        return w


# ---------------------------------------------------------------------------------------------------------------- slots, a second time
BLOCK = 256                   # lanes per workgroup of the list kernels
SHARE_CAP = 0.10
NO_NODE = 0xFFFFFFFF


def _step_to(spec, p, ax, d):
    """node ``p`` moved by d along ``ax`` -> (the node or None beyond a wall, the period crossed): a periodic axis wraps, any other ends"""
    q, n = list(p), spec.shape[ax]
    q[ax] += d
    if 0 <= q[ax] < n:
        return q, 0
    if spec.bc[ax][0] != BC_PERIODIC:
        return None, 0
    w = 1 if q[ax] >= n else -1
    q[ax] -= w * n
    return q, w


def kerr_slots(spec, a, ijk):
    """The slots of csrc/fdtd_nonlinear.hpp / spec.AnisoSet for E_a nodes ``ijk``, one node at a time: slots 0..3 component a + 1,
    4..7 component a + 2, at {i_a, i_a + 1} x {i_b - 1, i_b} (i_a runs first).
    -> (nbr_comp [8], nbr [n, 8, 3] with -1 for an empty slot, wrap [n, 8, 3])"""
    n = len(ijk)
    nbr, wrap = np.full((n, 8, 3), -1, np.int64), np.zeros((n, 8, 3), np.int64)
    comps = ((a + 1) % 3,) * 4 + ((a + 2) % 3,) * 4
    for e in range(n):
        slot = 0
        for b in ((a + 1) % 3, (a + 2) % 3):
            for db in (-1, 0):
                for da in (0, 1):
                    p, wa = _step_to(spec, [int(v) for v in ijk[e]], a, da)
                    if p is not None:
                        p, wb = _step_to(spec, p, b, db)
                    if p is not None:
                        nbr[e, slot] = p
                        wrap[e, slot, a], wrap[e, slot, b] = wa, wb
                    slot += 1
    return comps, nbr, wrap


def conformal_slots(spec, cs, unlisted_edges=True):
    """The slots of csrc/fdtd_conformal.hpp for the H faces of ``cs``, one face at a time: k = 0, 1 is E_a2 one node up along a1, then
    at the face's own index; k = 2, 3 is E_a1 one node up along a2, then at the face's own index.  Empty beyond a wall and, with
    ``unlisted_edges``, on an edge with l == 0.  -> (nbr_comp [4], nbr [n, 4, 3], wrap [n, 4, 3])"""
    c = cs.comp - 3
    a1, a2 = (c + 1) % 3, (c + 2) % 3
    n = len(cs.ijk)
    nbr, wrap = np.full((n, 4, 3), -1, np.int64), np.zeros((n, 4, 3), np.int64)
    for e in range(n):
        for k, (ax, d) in enumerate(((a1, 1), (a1, 0), (a2, 1), (a2, 0))):
            p, w = _step_to(spec, [int(v) for v in cs.ijk[e]], ax, d)
            if p is not None and not (unlisted_edges and cs.l[e, k] == 0.0):
                nbr[e, k], wrap[e, k, ax] = p, w
    return (a2, a2, a1, a1), nbr, wrap


def flat_table(shape, row, nbr):
    """[n, slots, 3] -> the [slots][n] uint32 rows the fdtd_add_* take: cell = (k ny + j) row + i, NO_NODE for an empty slot"""
    out = np.full((nbr.shape[1], nbr.shape[0]), NO_NODE, np.uint32)
    for e in range(nbr.shape[0]):
        for s in range(nbr.shape[1]):
            i, j, k = (int(v) for v in nbr[e, s])
            if i >= 0:
                out[s, e] = (k * shape[1] + j) * row + i
    return out


def presence(cls):
    """from the specs alone -> what the scenarios of the kind hold between them: a list with a full block and a tail, a list shorter than
    a wavefront, a listed node with an empty slot, one with a wrapped slot (``Scenario.slots_of``)"""
    out = {"n > 256, n % 256 != 0": [], "n < 64": [], "an empty slot": [], "a wrapped slot": []}
    for label in cls.all_labels():
        sc = scenario(cls, label)
        for s in sc.lists:
            n, nbr = len(s.ijk), sc.slots_of(s)[0]
            if n > BLOCK and n % BLOCK:
                out["n > 256, n % 256 != 0"].append((label, ds.COMP[s.comp], n))
            if n < 64:
                out["n < 64"].append((label, ds.COMP[s.comp], n))
            live = nbr[:, :, 0] >= 0
            if (~live).any():
                out["an empty slot"].append((label, ds.COMP[s.comp], int((~live).sum())))
            far = live & (np.abs(nbr - s.ijk[:, None, :]) > 1).any(axis=2)
            if far.any():
                out["a wrapped slot"].append((label, ds.COMP[s.comp], int(far.sum())))
    return out


# ---------------------------------------------------------------------------------------------------------------- planted deviations
def replace_list(spec, attr, n, **arrays):
    """``spec`` with list n of ``attr`` changed"""
    lists = list(getattr(spec, attr))
    lists[n] = dataclasses.replace(lists[n], **arrays)
    return dataclasses.replace(spec, **{attr: lists})


def scaled(s, name, index, rel):
    """{name: the list's coefficient array with element ``index`` times 1 + rel}"""
    a = np.array(getattr(s, name))
    a[index] = a[index] * (1.0 + rel)
    return {name: a}


def with_slot(s, e, slot, node):
    """{nbr_ijk: slot ``slot`` of entry e set to ``node`` (None: emptied)}"""
    nbr = np.array(s.nbr_ijk)
    nbr[e, slot] = -1 if node is None else node
    return {"nbr_ijk": nbr}


def value_at(fields, comp, node):
    return np.asarray(fields[comp])[node[..., 2], node[..., 1], node[..., 0]]


def slot_candidates(sc, s, kind):
    """per (entry, slot) of list ``s`` the size, in the STATE, of what plant ``kind`` changes in the sum the node reads — the plants go
    where the state makes them largest, which the reference alone decides:
      moved    the slot's node one further along x: |E(there) - E(slot)|, live slots whose moved node is in the grid
      emptied  |E(slot)|, live slots
      filled   |E(node across the wall)|, slots that a wall empties (not a PEC edge)
    -> (size [n, slots], the node each plant writes [n, slots, 3])"""
    nbr = np.asarray(s.nbr_ijk)
    live = nbr[:, :, 0] >= 0
    size, node = np.zeros(live.shape), np.full(nbr.shape, -1, np.int64)
    for slot in range(nbr.shape[1]):
        E = sc.state[s.nbr_comp[slot]]
        here = np.where(live[:, slot, None], nbr[:, slot], 0)
        if kind == "emptied":
            size[:, slot] = np.where(live[:, slot], np.abs(value_at([E], 0, here)), 0.0)
        elif kind == "moved":
            there = here.copy()
            there[:, 0] += 1
            ok = live[:, slot] & (there[:, 0] < sc.spec.shape[0])
            there = np.where(ok[:, None], there, 0)
            size[:, slot] = np.where(ok, np.abs(value_at([E], 0, there) - value_at([E], 0, here)), 0.0)
            node[:, slot] = there
        else:
            build = (lambda sp: kerr_slots(sp, s.comp, s.ijk)) if nbr.shape[1] == 8 else (lambda sp: conformal_slots(sp, s, False))
            opened = dataclasses.replace(sc.spec, bc=((BC_PERIODIC, BC_PERIODIC),) * 3)        # every wall opened: the node across it
            across = build(opened)[1][:, slot]
            walled = build(sc.spec)[1][:, slot, 0] < 0
            size[:, slot] = np.where(walled, np.abs(value_at([E], 0, across)), 0.0)
            node[:, slot] = across
    return size, node


def check_plant(sc, name, spec, named, *how):
    """The fp64 oracle of ``spec`` — ``sc.ref_spec(*how)`` with one list changed — against the clean one from the same state, at the
    smaller K of (1, 7) at which the plant acts.  -> (K, worst node, its bar, the whole-array rel-L2, is the worst node one of ``named``
    [(component, (i, j, k))])"""
    for K in (1, 7):
        clean, got = sc.ref(K, *how), sc._run(sc.ORACLE, spec, K)
        if any(not np.array_equal(a, b) for a, b in zip(clean, got)):
            break
    else:
        raise AssertionError(f"{sc.label}: plant {name} acts at neither K")
    w, bar = sc.measure(got, K, *how), sc.bar_nodes(K, *how)
    l2 = ds.rel_l2(ds.Run(clean, {}), ds.Run(got, {}))
    hit = (ds.COMP.index(w.comp), tuple(int(v) for v in w.index)) in {(int(c), tuple(int(v) for v in p)) for c, p in named}
    print(f"[plant] {sc.TAG} {sc.label} {name} K={K}: per node {w.value:.3e} = {w.value / bar:.1f} x bar {bar:.3e} | whole-array rel-L2 {l2:.3e} "
          f"(bar 2e-5) | names the planted node: {hit} | {w.at}")
    return K, w, bar, l2, hit


L2_BAR = 2e-5                 # the whole-array bar the plants are printed beside
FACTOR = 4.0                  # a plant stands at least this many bars high
RELS = (ds.REL, 1e-2, 1e-1)   # a coefficient plant steps up until it does; beyond 1e-1 the measure does not resolve the coefficient


def stands(sc, name, spec, named, *how, under_l2=False):
    K, w, bar, l2, hit = check_plant(sc, name, spec, named, *how)
    assert w.value >= FACTOR * bar, f"{sc.label} {name} K={K}: {w.value:.3e} is under {FACTOR:g} x the bar {bar:.3e}: {w}"
    assert hit, f"{sc.label} {name} K={K}: the worst node is not the planted one {named}: {w}"
    if under_l2:              # ... and the whole-array measure would have let it through
        assert l2 < L2_BAR, (sc.label, name, K, l2)
    return K, w, bar, l2


def resolved(sc, name, make, named, *how):
    """the smallest rel of RELS at which the coefficient plant stands; the value is the measure's resolution for that coefficient"""
    for rel in RELS:
        K, w, bar, l2, hit = check_plant(sc, f"{name} x (1 + {rel:g})", make(rel), named, *how)
        if w.value >= FACTOR * bar and hit:
            print(f"[plant] {sc.TAG} {sc.label} {name}: resolved at rel {rel:g}")
            return rel, l2
    raise AssertionError(f"{sc.label} {name}: not resolvable by the per-node measure up to rel {RELS[-1]:g}")


def best(size):
    """(entry, slot) of the candidate at the median of the non-zero sizes: a node like most, chosen by the state alone — the largest
    candidate is also the one the whole-array figure sees best"""
    flat = np.flatnonzero(size.reshape(-1) > 0)
    assert flat.size
    pick = flat[np.argsort(size.reshape(-1)[flat], kind="stable")[flat.size // 2]]
    e, slot = np.unravel_index(int(pick), size.shape)
    return int(e), int(slot)


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
