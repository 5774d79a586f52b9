"""tidy3d-compatible ``.hdf5`` files without h5py: a thin ctypes binding of the HDF5 C library.

SURVEY.md section 8(f) rank 1: results must flow into ``tidy3d.SimulationData.from_file`` /
``web.load``-style workflows.  The reference writes its files with h5py (ref components/base.py:691-738
``to_hdf5``, data/data_array.py:248-267 ``to_hdf5_handle``); the layout is plain HDF5:

* ``/JSON_STRING`` (``JSON_STRING_1`` ... when longer than 1e9 chars): scalar variable-length UTF-8
  string — the model's JSON with every DataArray replaced by its class name (ref base.py:183-188,
  :904-930);
* one group per DataArray at the key path of that field (tuples use the element index as group
  name, ref base.py:537-549), holding ``__xarray_dataarray_variable__`` (values; complex stored the
  h5py way, a compound ``{r, i}``) and one dataset per coordinate (strings: variable-length UTF-8).

h5py is not installable here, the C library is present (``libhdf5.so``, 1.10): this module binds the
handful of entry points needed.  Files written here are read back by h5py exactly as the reference
does it (tests/test_hdf5.py runs the reference's own read recipe under a python that has h5py).
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import glob
import json
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .exceptions import Tidy3dNotImplementedError

DATA_ARRAY_VALUE_NAME = "__xarray_dataarray_variable__"     # ref data/data_array.py:60
JSON_TAG = "JSON_STRING"                                      # ref base.py:35
MAX_STRING_LENGTH = 1_000_000_000                              # ref base.py:37

hid_t = C.c_int64
hsize_t = C.c_uint64
H5P_DEFAULT = 0
H5S_ALL = 0
H5F_ACC_RDONLY, H5F_ACC_TRUNC = 0, 2
H5S_SCALAR = 0
H5T_VARIABLE = C.c_size_t(-1).value
H5T_CSET_UTF8 = 1
H5T_FLOAT, H5T_INTEGER, H5T_STRING, H5T_COMPOUND = 1, 0, 3, 6
H5G_GROUP, H5G_DATASET = 0, 1


def _find_library() -> Optional[str]:
    cands = [os.environ.get("TIDY3D_AMD_HDF5"), ctypes.util.find_library("hdf5")]
    for pat in ("/opt/conda/lib/libhdf5.so*", "/usr/lib/x86_64-linux-gnu/libhdf5*.so*",
                "/usr/lib/x86_64-linux-gnu/hdf5/serial/libhdf5.so*", "/usr/local/lib/libhdf5.so*"):
        cands += sorted(p for p in glob.glob(pat) if "_hl" not in p and "_cpp" not in p and "fortran" not in p)
    for c in cands:
        if not c:
            continue
        try:
            C.CDLL(c)
            return c
        except OSError:
            continue
    return None


class Hdf5Library:
    """The bound C library (one per process)."""

    _inst: Optional["Hdf5Library"] = None

    @classmethod
    def get(cls) -> "Hdf5Library":
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def __init__(self):
        path = _find_library()
        if path is None:
            raise Tidy3dNotImplementedError(
                "writing / reading .hdf5 needs the HDF5 C library (libhdf5.so; set TIDY3D_AMD_HDF5 to its "
                "path) — use a .npz path otherwise")
        self.path = path
        L = self.L = C.CDLL(path)

        def sig(name, res, *args):
            f = getattr(L, name)
            f.restype, f.argtypes = res, list(args)
            return f
        i, cp, vp = C.c_int, C.c_char_p, C.c_void_p
        sig("H5open", i)
        sig("H5Fcreate", hid_t, cp, C.c_uint, hid_t, hid_t)
        sig("H5Fopen", hid_t, cp, C.c_uint, hid_t)
        sig("H5Fclose", i, hid_t)
        sig("H5Gcreate2", hid_t, hid_t, cp, hid_t, hid_t, hid_t)
        sig("H5Gopen2", hid_t, hid_t, cp, hid_t)
        sig("H5Gclose", i, hid_t)
        sig("H5Gget_num_objs", i, hid_t, C.POINTER(hsize_t))
        sig("H5Gget_objname_by_idx", C.c_ssize_t, hid_t, hsize_t, cp, C.c_size_t)
        sig("H5Gget_objtype_by_idx", i, hid_t, hsize_t)
        sig("H5Screate", hid_t, i)
        sig("H5Screate_simple", hid_t, i, C.POINTER(hsize_t), C.POINTER(hsize_t))
        sig("H5Sclose", i, hid_t)
        sig("H5Sget_simple_extent_ndims", i, hid_t)
        sig("H5Sget_simple_extent_dims", i, hid_t, C.POINTER(hsize_t), C.POINTER(hsize_t))
        sig("H5Dcreate2", hid_t, hid_t, cp, hid_t, hid_t, hid_t, hid_t, hid_t)
        sig("H5Dopen2", hid_t, hid_t, cp, hid_t)
        sig("H5Dwrite", i, hid_t, hid_t, hid_t, hid_t, hid_t, vp)
        sig("H5Dread", i, hid_t, hid_t, hid_t, hid_t, hid_t, vp)
        sig("H5Dget_type", hid_t, hid_t)
        sig("H5Dget_space", hid_t, hid_t)
        sig("H5Dclose", i, hid_t)
        sig("H5Dvlen_reclaim", i, hid_t, hid_t, hid_t, vp)
        sig("H5Tcopy", hid_t, hid_t)
        sig("H5Tcreate", hid_t, i, C.c_size_t)
        sig("H5Tinsert", i, hid_t, cp, C.c_size_t, hid_t)
        sig("H5Tset_size", i, hid_t, C.c_size_t)
        sig("H5Tset_cset", i, hid_t, i)
        sig("H5Tget_class", i, hid_t)
        sig("H5Tget_size", C.c_size_t, hid_t)
        sig("H5Tis_variable_str", i, hid_t)
        sig("H5Tget_nmembers", i, hid_t)
        sig("H5Tget_member_type", hid_t, hid_t, C.c_uint)
        sig("H5Tclose", i, hid_t)
        sig("H5Eset_auto2", i, hid_t, vp, vp)
        if L.H5open() < 0:
            raise OSError("H5open failed")
        L.H5Eset_auto2(0, None, None)          # errors are reported through return codes below

        def glob_id(name):
            return hid_t.in_dll(L, name).value
        self.F32, self.F64 = glob_id("H5T_IEEE_F32LE_g"), glob_id("H5T_IEEE_F64LE_g")
        self.I32, self.I64 = glob_id("H5T_STD_I32LE_g"), glob_id("H5T_STD_I64LE_g")
        self.U8 = glob_id("H5T_STD_U8LE_g")
        self.C_S1 = glob_id("H5T_C_S1_g")
        self.vstr = L.H5Tcopy(self.C_S1)
        L.H5Tset_size(self.vstr, H5T_VARIABLE)
        L.H5Tset_cset(self.vstr, H5T_CSET_UTF8)
        self.c64 = self._complex_type(self.F32, 4)
        self.c128 = self._complex_type(self.F64, 8)

    def _complex_type(self, base: int, size: int) -> int:
        t = self.L.H5Tcreate(H5T_COMPOUND, 2 * size)      # h5py's complex: {"r": float, "i": float}
        self.L.H5Tinsert(t, b"r", 0, base)
        self.L.H5Tinsert(t, b"i", size, base)
        return t

    def _np_type(self, dt: np.dtype) -> int:
        table = {np.dtype("<f4"): self.F32, np.dtype("<f8"): self.F64, np.dtype("<i4"): self.I32,
                 np.dtype("<i8"): self.I64, np.dtype("u1"): self.U8, np.dtype("<c8"): self.c64,
                 np.dtype("<c16"): self.c128, np.dtype(bool): self.U8}
        if dt not in table:
            raise TypeError(f"no HDF5 type for numpy dtype {dt}")
        return table[dt]


def _chk(v: int, what: str) -> int:
    if v < 0:
        raise OSError(f"HDF5: {what} failed")
    return v


class H5Writer:
    def __init__(self, path: str):
        self.h = Hdf5Library.get()
        self.fid = _chk(self.h.L.H5Fcreate(os.fsencode(path), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT), f"create {path}")

    def close(self):
        if self.fid:
            self.h.L.H5Fclose(self.fid)
            self.fid = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _parent(self, path: str) -> Tuple[int, bytes, List[int]]:
        """Create intermediate groups; returns (location id, leaf name, groups to close)."""
        parts = [p for p in path.split("/") if p]
        loc, opened = self.fid, []
        for p in parts[:-1]:
            g = self.h.L.H5Gopen2(loc, p.encode(), H5P_DEFAULT)
            if g < 0:
                g = _chk(self.h.L.H5Gcreate2(loc, p.encode(), H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"group {p}")
            opened.append(g)
            loc = g
        return loc, parts[-1].encode(), opened

    def _close_all(self, ids):
        for g in reversed(ids):
            self.h.L.H5Gclose(g)

    def group(self, path: str):
        loc, leaf, opened = self._parent(path)
        g = self.h.L.H5Gopen2(loc, leaf, H5P_DEFAULT)
        if g < 0:
            g = _chk(self.h.L.H5Gcreate2(loc, leaf, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"group {path}")
        self.h.L.H5Gclose(g)
        self._close_all(opened)

    def array(self, path: str, arr) -> None:
        a = np.ascontiguousarray(arr)
        if a.dtype.kind in "US" or a.dtype == object:
            return self.strings(path, [str(s) for s in a.ravel().tolist()], shape=a.shape)
        if a.dtype.byteorder == ">":
            a = a.astype(a.dtype.newbyteorder("<"))
        L = self.h.L
        ftype = self.h._np_type(a.dtype)
        if a.ndim == 0:
            space = L.H5Screate(H5S_SCALAR)
        else:
            dims = (hsize_t * a.ndim)(*a.shape)
            space = L.H5Screate_simple(a.ndim, dims, None)
        loc, leaf, opened = self._parent(path)
        d = _chk(L.H5Dcreate2(loc, leaf, ftype, space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"dataset {path}")
        if a.size:
            _chk(L.H5Dwrite(d, ftype, H5S_ALL, H5S_ALL, H5P_DEFAULT, a.ctypes.data_as(C.c_void_p)), f"write {path}")
        L.H5Dclose(d)
        L.H5Sclose(space)
        self._close_all(opened)

    def string(self, path: str, text: str) -> None:
        """Scalar variable-length UTF-8 string (what h5py stores for ``group[key] = "..."``)."""
        L = self.h.L
        space = L.H5Screate(H5S_SCALAR)
        loc, leaf, opened = self._parent(path)
        d = _chk(L.H5Dcreate2(loc, leaf, self.h.vstr, space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"dataset {path}")
        buf = (C.c_char_p * 1)(text.encode("utf-8"))
        _chk(L.H5Dwrite(d, self.h.vstr, H5S_ALL, H5S_ALL, H5P_DEFAULT, C.cast(buf, C.c_void_p)), f"write {path}")
        L.H5Dclose(d)
        L.H5Sclose(space)
        self._close_all(opened)

    def strings(self, path: str, items: List[str], shape=None) -> None:
        L = self.h.L
        shape = tuple(shape) if shape is not None else (len(items),)
        dims = (hsize_t * len(shape))(*shape)
        space = L.H5Screate_simple(len(shape), dims, None)
        loc, leaf, opened = self._parent(path)
        d = _chk(L.H5Dcreate2(loc, leaf, self.h.vstr, space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"dataset {path}")
        buf = (C.c_char_p * max(len(items), 1))(*[s.encode("utf-8") for s in items])
        if items:
            _chk(L.H5Dwrite(d, self.h.vstr, H5S_ALL, H5S_ALL, H5P_DEFAULT, C.cast(buf, C.c_void_p)), f"write {path}")
        L.H5Dclose(d)
        L.H5Sclose(space)
        self._close_all(opened)


def read_tree(path: str) -> Dict[str, Any]:
    """Whole file as {"/group/dataset": ndarray | str | list[str]} (testing / loading aid)."""
    h = Hdf5Library.get()
    L = h.L
    fid = _chk(L.H5Fopen(os.fsencode(path), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    out: Dict[str, Any] = {}

    def read_dataset(loc, name: bytes):
        d = _chk(L.H5Dopen2(loc, name, H5P_DEFAULT), "open dataset")
        t, s = L.H5Dget_type(d), L.H5Dget_space(d)
        nd = L.H5Sget_simple_extent_ndims(s)
        dims = (hsize_t * max(nd, 1))()
        if nd > 0:
            L.H5Sget_simple_extent_dims(s, dims, None)
        shape = tuple(int(dims[k]) for k in range(nd))
        n = int(np.prod(shape)) if nd else 1
        cls, size = L.H5Tget_class(t), L.H5Tget_size(t)
        if cls == H5T_STRING:
            if not L.H5Tis_variable_str(t):
                raise TypeError("fixed-length strings are not used by tidy3d files")
            buf = (C.c_char_p * n)()
            _chk(L.H5Dread(d, h.vstr, H5S_ALL, H5S_ALL, H5P_DEFAULT, C.cast(buf, C.c_void_p)), "read")
            vals = [(b or b"").decode("utf-8") for b in buf]
            L.H5Dvlen_reclaim(h.vstr, s, H5P_DEFAULT, C.cast(buf, C.c_void_p))
            res = vals[0] if nd == 0 else vals
        else:
            if cls == H5T_FLOAT:
                dt, mem = (np.dtype("<f4"), h.F32) if size == 4 else (np.dtype("<f8"), h.F64)
            elif cls == H5T_INTEGER:
                dt, mem = {1: (np.dtype("u1"), h.U8), 4: (np.dtype("<i4"), h.I32), 8: (np.dtype("<i8"), h.I64)}[size]
            elif cls == H5T_COMPOUND and L.H5Tget_nmembers(t) == 2:
                dt, mem = (np.dtype("<c8"), h.c64) if size == 8 else (np.dtype("<c16"), h.c128)
            else:
                raise TypeError(f"unsupported HDF5 type class {cls}")
            res = np.empty(shape, dtype=dt)
            if res.size:
                _chk(L.H5Dread(d, mem, H5S_ALL, H5S_ALL, H5P_DEFAULT, res.ctypes.data_as(C.c_void_p)), "read")
        L.H5Tclose(t)
        L.H5Sclose(s)
        L.H5Dclose(d)
        return res

    def walk(loc, prefix: str):
        n = hsize_t(0)
        L.H5Gget_num_objs(loc, C.byref(n))
        for idx in range(n.value):
            ln = L.H5Gget_objname_by_idx(loc, idx, None, 0)
            buf = C.create_string_buffer(ln + 1)
            L.H5Gget_objname_by_idx(loc, idx, buf, ln + 1)
            name = buf.value
            kind = L.H5Gget_objtype_by_idx(loc, idx)
            full = f"{prefix}/{name.decode()}"
            if kind == H5G_GROUP:
                g = L.H5Gopen2(loc, name, H5P_DEFAULT)
                out.setdefault(full + "/", None)
                walk(g, full)
                L.H5Gclose(g)
            elif kind == H5G_DATASET:
                out[full] = read_dataset(loc, name)

    root = L.H5Gopen2(fid, b"/", H5P_DEFAULT)
    walk(root, "")
    L.H5Gclose(root)
    L.H5Fclose(fid)
    return out


# ----------------------------------------------------------------------------------------------
# SimulationData <-> file
# ----------------------------------------------------------------------------------------------

_ARRAY_TYPES = {          # container field -> tidy3d DataArray class name (ref data/data_array.py DATA_ARRAY_MAP)
    "FieldData": "ScalarFieldDataArray", "FieldTimeData": "ScalarFieldTimeDataArray",
    "PermittivityData": "ScalarFieldDataArray",
}


def surface_name(mon, sname: str) -> str:
    """Name the reference gives the near-field surface monitors (ref monitor.py:518-566)."""
    return mon.name if sname == "plane" else f"{mon.name}_{sname}"


def _grid_json(ge: Dict[str, np.ndarray]) -> dict:
    return {"type": "Grid", "boundaries": {"type": "Coords", **{d: np.asarray(ge[d], float).tolist() for d in "xyz"}}}


def _monitor_json(sim_data, mon) -> dict:
    src = getattr(sim_data.simulation, "_source_dict", None)
    if src:
        for m in src.get("monitors", ()):
            if m.get("name") == mon.name:
                return m
    return mon.dict()


# dims of the reference's DataArray classes that describe a Simulation (ref data/data_array.py)
SIM_ARRAY_DIMS = {"SpatialDataArray": ("x", "y", "z"), "ScalarFieldDataArray": ("x", "y", "z", "f"),
                  "TimeDataArray": ("t",), "TriangleMeshDataArray": ("face_index", "vertex_index", "axis"),
                  "PointDataArray": ("index", "axis"), "IndexedDataArray": ("index",), "CellDataArray": ("cell_index", "vertex_index")}


def _split_arrays(node, path: str, arrays: Dict[str, Any]):
    """Copy of a JSON-like tree with every DataArray replaced by its class tag; the arrays are collected
    under their hdf5 group path."""
    from .data import DataArray
    if isinstance(node, DataArray):
        arrays[path] = node
        return getattr(node, "tag", None) or "DataArray"
    if isinstance(node, dict):
        return {k: _split_arrays(v, f"{path}/{k}", arrays) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_split_arrays(v, f"{path}/{i}", arrays) for i, v in enumerate(node)]
    return node


def _join_arrays(node, path: str, tree: Dict[str, Any]):
    """Inverse of ``_split_arrays`` on a tree read from an hdf5 file: "...DataArray" placeholders whose group
    holds a value dataset become DataArrays (dims from SIM_ARRAY_DIMS, else matched by length)."""
    from .data import DataArray
    if isinstance(node, dict):
        return {k: _join_arrays(v, f"{path}/{k}", tree) for k, v in node.items()}
    if isinstance(node, list):
        return [_join_arrays(v, f"{path}/{i}", tree) for i, v in enumerate(node)]
    if isinstance(node, str) and node.endswith("DataArray") and f"{path}/{DATA_ARRAY_VALUE_NAME}" in tree:
        values = np.asarray(tree[f"{path}/{DATA_ARRAY_VALUE_NAME}"])
        names = [k[len(path) + 1:] for k in tree if k.startswith(path + "/") and "/" not in k[len(path) + 1:]
                 and k != f"{path}/{DATA_ARRAY_VALUE_NAME}" and tree[k] is not None]
        dims = SIM_ARRAY_DIMS.get(node)
        if dims is None or len(dims) != values.ndim:
            dims, left = [], list(names)
            for i_d, n in enumerate(values.shape):
                pick = next((d for d in left if len(np.atleast_1d(tree[f"{path}/{d}"])) == n), f"dim_{i_d}")
                dims.append(pick)
                if pick in left:
                    left.remove(pick)
        coords = {d: (np.atleast_1d(np.asarray(tree[f"{path}/{d}"])) if tree.get(f"{path}/{d}") is not None
                      else np.arange(values.shape[i_d])) for i_d, d in enumerate(dims)}
        arr = DataArray(values, coords)
        arr.tag = node
        return arr
    return node


def load_simulation(path: str):
    """Read a ``tidy3d.Simulation`` from an .hdf5 file written by the reference's ``to_file`` / ``to_hdf5``
    (ref base.py:560-738) or from a SimulationData file: unlike the JSON form, datasets (custom media and
    sources, triangle meshes, custom source times) come along."""
    from . import schema as td
    tree = read_tree(path)
    keys = sorted((k for k in tree if k.lstrip("/").split("_")[0] == "JSON" and k.lstrip("/").startswith(JSON_TAG)),
                  key=lambda k: int(k.rsplit("_", 1)[1]) if k.lstrip("/") != JSON_TAG else 0)
    model = json.loads("".join(tree[k] for k in keys))
    base = ""
    if model.get("type") == "SimulationData":
        model, base = model["simulation"], "/simulation"
    return td.Simulation.from_dict(_join_arrays(model, base, tree))


def simulation_data_model(sim_data) -> Tuple[dict, Dict[str, Any]]:
    """(JSON model with DataArray placeholders, {hdf5 group path: DataArray}) of a SimulationData in
    the reference's layout (ref sim_data.py:826, monitor_data.py)."""
    sim = sim_data.simulation
    arrays: Dict[str, Any] = {}
    # dataset-defined objects of the simulation (custom media / sources, triangle meshes): placeholders in
    # the JSON, arrays under the same path (ref base.py:691-738 to_hdf5)
    sim_json = _split_arrays(getattr(sim, "_source_dict", None) or sim.dict(), "/simulation", arrays)
    data_json = []
    for i, d in enumerate(sim_data.data):
        kind = type(d).__name__
        entry = {"type": kind, "monitor": _monitor_json(sim_data, d.monitor)}
        base = f"/data/{i}"
        if kind in ("FieldData", "FieldTimeData", "PermittivityData"):
            entry["symmetry"] = [0, 0, 0]
            entry["symmetry_center"] = [float(v) for v in sim.center]
            entry["grid_expanded"] = _grid_json(d.grid_expanded)
            for name, arr in d.field_components.items():
                if arr is None:
                    continue
                entry[name] = _ARRAY_TYPES[kind]
                arrays[f"{base}/{name}"] = arr
        elif kind in ("FluxData", "FluxTimeData"):
            entry["flux"] = "FluxDataArray" if kind == "FluxData" else "FluxTimeDataArray"
            arrays[f"{base}/flux"] = d.flux
        elif kind == "ModeData":
            entry["amps"], entry["n_complex"] = "ModeAmpsDataArray", "ModeIndexDataArray"
            arrays[f"{base}/amps"], arrays[f"{base}/n_complex"] = d.amps, d.n_complex
            # mode_power (the flux a unit-amplitude mode carries as this monitor measures it; not a field of the
            # reference's ModeData): an extra DataArray group beside the two the JSON model names — the reference's
            # loader never looks at it, this package's reader picks it up
            if getattr(d, "mode_power", None) is not None:
                arrays[f"{base}/mode_power"] = d.mode_power
        elif kind == "ModeSolverData":
            # ref monitor_data.py ModeSolverData: six ScalarModeFieldDataArrays + n_complex
            entry["symmetry"] = [0, 0, 0]
            entry["symmetry_center"] = [float(v) for v in sim.center]
            entry["grid_expanded"] = _grid_json(d.grid_expanded)
            entry["n_complex"] = "ModeIndexDataArray"
            arrays[f"{base}/n_complex"] = d.n_complex
            for name, arr in d.field_components.items():
                entry[name] = "ScalarModeFieldDataArray"
                arrays[f"{base}/{name}"] = arr
        elif kind in ("FieldProjectionAngleData", "FieldProjectionCartesianData", "FieldProjectionKSpaceData", "DirectivityData"):
            from .discretize import flux_surfaces
            mon = d.monitor
            # ref monitor.py:874-889: the near-field surfaces as colocated FieldMonitors
            entry["projection_surfaces"] = [
                {"type": "FieldProjectionSurface", "normal_dir": "+" if sign > 0 else "-",
                 "monitor": {"type": "FieldMonitor", "center": [float(c) for c in box.center],
                             "size": [float(c) for c in box.size], "freqs": [float(f) for f in mon.freqs],
                             "name": surface_name(mon, sname), "colocate": True}}
                for sname, box, axis, sign in flux_surfaces(mon)]
            entry["medium"] = (mon.medium if mon.medium is not None else sim.medium).dict()
            entry["is_2d_simulation"] = False
            for name, arr in d.field_components.items():      # (DirectivityData: the angle-data group plus a flux array)
                entry[name] = "FieldProjectionAngleDataArray" if kind == "DirectivityData" else kind.replace("Data", "DataArray")
                arrays[f"{base}/{name}"] = arr
            if kind == "DirectivityData":
                entry["flux"] = "FluxDataArray"
                arrays[f"{base}/flux"] = d.flux
        elif kind == "DiffractionData":
            # ref monitor_data.py:2672-2751: six DiffractionDataArrays + sim_size, bloch_vecs, medium
            entry["sim_size"] = [float(v) for v in d.sim_size]
            entry["bloch_vecs"] = [float(v) for v in d.bloch_vecs]
            entry["medium"] = d.medium.dict()
            entry["is_2d_simulation"] = False
            for name, arr in d.field_components.items():
                entry[name] = "DiffractionDataArray"
                arrays[f"{base}/{name}"] = arr
        else:
            raise Tidy3dNotImplementedError(f"no hdf5 layout for {kind}")
        data_json.append(entry)
    model = {"type": "SimulationData", "simulation": sim_json, "data": data_json,
             "log": sim_data.log, "diverged": bool(sim_data.diverged)}
    return model, arrays


def write_simulation_data(sim_data, path: str) -> None:
    """``SimulationData.to_file(path.hdf5)`` of the reference, from the mirror containers."""
    model, arrays = simulation_data_model(sim_data)
    def default(o):
        if isinstance(o, np.generic):
            return o.item()
        if isinstance(o, np.ndarray):
            return o.tolist()
        if isinstance(o, complex):
            return {"real": o.real, "imag": o.imag}
        raise TypeError(f"{type(o).__name__} is not JSON serialisable")

    text = json.dumps(model, default=default)
    with H5Writer(path) as w:
        for ind in range(max(1, -(-len(text) // MAX_STRING_LENGTH))):
            key = JSON_TAG if ind == 0 else f"{JSON_TAG}_{ind}"
            w.string("/" + key, text[ind * MAX_STRING_LENGTH:(ind + 1) * MAX_STRING_LENGTH])
        for gpath, arr in arrays.items():
            w.group(gpath)
            w.array(f"{gpath}/{DATA_ARRAY_VALUE_NAME}", np.asarray(arr.values))
            for dim in arr.dims:
                w.array(f"{gpath}/{dim}", np.asarray(arr.coords[dim]))


def load_simulation_data(path: str):
    """Read a file written by ``write_simulation_data`` (or by the reference, for the data types
    the mirror has) back into the mirror containers."""
    from . import schema as td
    from .data import (DataArray, FieldData, FieldTimeData, FluxData, FluxTimeData, PermittivityData,
                       SimulationData)
    from .modesource import ModeData
    tree = read_tree(path)
    keys = sorted((k for k in tree if k.lstrip("/").startswith(JSON_TAG) and not k.endswith("/")),
                  key=lambda k: int(k.rsplit("_", 1)[1]) if k.lstrip("/") != JSON_TAG else 0)
    model = json.loads("".join(tree[k] for k in keys))
    sim = td.Simulation.from_dict(_join_arrays(model["simulation"], "/simulation", tree))
    by_name = {m.name: m for m in sim.monitors}
    dims = {"ScalarFieldDataArray": ("x", "y", "z", "f"), "ScalarFieldTimeDataArray": ("x", "y", "z", "t"),
            "FluxDataArray": ("f",), "FluxTimeDataArray": ("t",), "ModeAmpsDataArray": ("direction", "f", "mode_index"),
            "ModeIndexDataArray": ("f", "mode_index"),
            "ScalarModeFieldDataArray": ("x", "y", "z", "f", "mode_index"),
            "FieldProjectionAngleDataArray": ("r", "theta", "phi", "f"),
            "FieldProjectionCartesianDataArray": ("x", "y", "z", "f"),
            "FieldProjectionKSpaceDataArray": ("ux", "uy", "r", "f"),
            "DiffractionDataArray": ("orders_x", "orders_y", "f")}

    def arr(gpath: str, tag: str) -> DataArray:
        coords = {d: (np.asarray(tree[f"{gpath}/{d}"]) if not isinstance(tree[f"{gpath}/{d}"], list)
                      else list(tree[f"{gpath}/{d}"])) for d in dims[tag]}
        return DataArray(tree[f"{gpath}/{DATA_ARRAY_VALUE_NAME}"], coords)

    out = []
    for i, e in enumerate(model["data"]):
        mon = by_name[e["monitor"]["name"]]
        base = f"/data/{i}"
        kind = e["type"]
        fields = {k: arr(f"{base}/{k}", v) for k, v in e.items() if isinstance(v, str) and v in dims}
        if kind in ("FieldData", "FieldTimeData"):
            ge = {d: np.asarray(e["grid_expanded"]["boundaries"][d]) for d in "xyz"}
            cls = FieldData if kind == "FieldData" else FieldTimeData
            out.append(cls(monitor=mon, symmetry=tuple(e.get("symmetry", (0, 0, 0))),
                           symmetry_center=tuple(e.get("symmetry_center") or sim.center), grid_expanded=ge, **fields))
        elif kind == "PermittivityData":
            ge = {d: np.asarray(e["grid_expanded"]["boundaries"][d]) for d in "xyz"}
            out.append(PermittivityData(monitor=mon, grid_expanded=ge, **fields))
        elif kind == "FluxData":
            out.append(FluxData(monitor=mon, flux=fields["flux"]))
        elif kind == "FluxTimeData":
            out.append(FluxTimeData(monitor=mon, flux=fields["flux"]))
        elif kind == "ModeData":
            mp = arr(f"{base}/mode_power", "ModeAmpsDataArray") if f"{base}/mode_power/{DATA_ARRAY_VALUE_NAME}" in tree else None
            out.append(ModeData(monitor=mon, amps=fields["amps"], n_complex=fields["n_complex"], mode_power=mp))
        elif kind == "ModeSolverData":
            from .plugins.mode import ModeSolverData
            out.append(ModeSolverData(monitor=mon, grid_expanded={d: np.asarray(e["grid_expanded"]["boundaries"][d])
                                                                  for d in "xyz"}, **fields))
        elif kind in ("FieldProjectionAngleData", "FieldProjectionCartesianData", "FieldProjectionKSpaceData"):
            from . import projection
            out.append(getattr(projection, kind)(monitor=mon, **fields))
        elif kind == "DirectivityData":
            from .data import DirectivityData
            out.append(DirectivityData(monitor=mon, **fields))
        elif kind == "DiffractionData":
            from . import projection
            out.append(projection.DiffractionData(monitor=mon, sim_size=tuple(e["sim_size"]),
                                                  bloch_vecs=tuple(e["bloch_vecs"]), medium=td.parse(e["medium"]), **fields))
        else:
            raise Tidy3dNotImplementedError(f"no mirror container for {kind}")
    return SimulationData(simulation=sim, data=tuple(out), log=model.get("log") or "",
                          diverged=bool(model.get("diverged", False)))
