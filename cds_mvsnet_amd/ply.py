"""PLY files: one header parser, one header writer, and the project's readers and writers of clouds and meshes on top of them.

A header is a format and a list of elements ``(name, count, properties)``; a property is ``(name, type)`` or, for a list
property, ``(name, (count type, item type))``, the types as numpy codes without byte order ("f4", "u1", ...).
:func:`read_header` parses that form and :func:`header_bytes` writes it, so a strict reader states the layout it accepts as
a comparison with the layout its writer puts out."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}
_NAMES = {"f4": "float", "u1": "uchar", "i4": "int"}           # the names the writers use
_FORMATS = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}
LITTLE = "binary_little_endian"

XYZ = [("x", "f4"), ("y", "f4"), ("z", "f4")]
NORMAL = [("nx", "f4"), ("ny", "f4"), ("nz", "f4")]
RGB = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
TRIANGLES = [("vertex_indices", ("u1", "i4"))]


def _type(t: str, path: str) -> str:
    if t not in _TYPES:
        raise ValueError(f"{path}: unknown PLY type {t}")
    return _TYPES[t]


def read_header(f, path: str) -> Tuple[str, List[tuple]]:
    """The header of the PLY file open (binary) at ``f`` -> (format, [(element, count, properties)]); ``f`` is left at the
    first byte of the data.  ``comment`` and ``obj_info`` lines are skipped."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: PLY header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], (_type(tok[2], path), _type(tok[3], path))))
            else:
                elements[-1][2].append((tok[2], _type(tok[1], path)))
    if fmt not in _FORMATS:
        raise ValueError(f"{path}: unsupported PLY format {fmt}")
    return fmt, elements


def header_bytes(elements) -> bytes:
    """[(element, count, properties)] -> the binary little-endian header the writers put out."""
    lines = ["ply", f"format {LITTLE} 1.0"]
    for name, count, props in elements:
        lines.append(f"element {name} {count}")
        lines += [f"property list {_NAMES[t[0]]} {_NAMES[t[1]]} {p}" if isinstance(t, tuple) else f"property {_NAMES[t]} {p}"
                  for p, t in props]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def _dtype(props, end: str = "<", list_len: Optional[int] = None) -> np.dtype:
    """The record of one row of an element; a list property (only with ``list_len``, the one length of every row) is its
    count ``<name>.n`` and its items."""
    fields = []
    for p, t in props:
        fields += [(p + ".n", end + t[0]), (p, end + t[1], (list_len,))] if isinstance(t, tuple) else [(p, end + t)]
    return np.dtype(fields)


def _records(props, n: int, columns, list_len: Optional[int] = None) -> np.ndarray:
    """``n`` rows of an element, filled from ``columns``: [(property names, array [n, len(names)])]."""
    rec = np.empty(n, dtype=_dtype(props, "<", list_len))
    for names, a in columns:
        for i, name in enumerate(names):
            rec[name] = a[:, i]
    return rec


def _write(path: str, elements, records) -> None:
    with open(path, "wb") as f:
        f.write(header_bytes(elements))
        for rec in records:
            rec.tofile(f)


def _read_records(f, path: str, props, n: int, list_len: Optional[int] = None) -> np.ndarray:
    dt = _dtype(props, "<", list_len)
    raw = f.read(dt.itemsize * n)
    if len(raw) != dt.itemsize * n:
        raise ValueError(f"{path}: truncated")
    return np.frombuffer(raw, dtype=dt, count=n)


def _columns(rec: np.ndarray, names) -> np.ndarray:
    return np.stack([rec[c] for c in names], -1).reshape(len(rec), len(names))


# --------------------------------------------------------------------------------------------------------------- clouds
def write_ply(path: str, points: np.ndarray, colors: np.ndarray, normals: Optional[np.ndarray] = None) -> None:
    """Binary little-endian PLY with x,y,z float32 + red,green,blue uint8 vertices (what plyfile writes in
    test.py:370-382).  With ``normals`` [N,3] the vertex is x y z nx ny nz red green blue, the order Open3D and MeshLab write."""
    n = int(points.shape[0])
    if normals is not None and tuple(normals.shape) != (n, 3):
        raise ValueError(f"write_ply: {tuple(normals.shape)} normals for {n} points")
    props = XYZ + (NORMAL if normals is not None else []) + RGB
    columns = [("xyz", points), (("red", "green", "blue"), colors)] + ([(("nx", "ny", "nz"), normals)] if normals is not None else [])
    _write(path, [("vertex", n, props)], [_records(props, n, columns)])


def read_ply_full(path: str) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """A PLY written by :func:`write_ply`, with or without normals -> (points float32 [N,3], colors uint8 [N,3],
    normals float32 [N,3] | None).  ValueError for any other layout."""
    with open(path, "rb") as f:
        fmt, elements = read_header(f, path)
        props = elements[0][2] if len(elements) == 1 and elements[0][0] == "vertex" else None
        if fmt != LITTLE or props not in (XYZ + RGB, XYZ + NORMAL + RGB):
            raise ValueError(f"{path}: not a vertex layout that write_ply produces: {props}")
        rec = _read_records(f, path, props, elements[0][1])
    return _columns(rec, "xyz"), _columns(rec, ("red", "green", "blue")), \
        _columns(rec, ("nx", "ny", "nz")) if len(props) == 9 else None


def read_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(points, colors) of :func:`read_ply_full`.  It used to assume ``x y z red green blue`` whatever the header declared: a
    file with normals now gives its points and colours instead of misaligned bytes, and any other layout raises."""
    return read_ply_full(path)[:2]


# --------------------------------------------------------------------------------------------------------------- meshes
def write_mesh_ply(path: str, vertices: np.ndarray, colors: np.ndarray, faces: np.ndarray) -> None:
    """Binary little-endian PLY: vertex x y z red green blue, face ``property list uchar int vertex_indices`` (triangles).
    No normals: viewers derive them from the winding."""
    vertices, colors, faces = np.asarray(vertices), np.asarray(colors), np.asarray(faces)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if tuple(vertices.shape) != (nv, 3) or tuple(colors.shape) != (nv, 3) or tuple(faces.shape) != (nf, 3):
        raise ValueError(f"write_mesh_ply: vertices [V,3], colors [V,3], faces [F,3] expected, got {vertices.shape}, {colors.shape}, "
                         f"{faces.shape}")
    if nf and (int(faces.min()) < 0 or int(faces.max()) >= nv):
        raise ValueError(f"write_mesh_ply: faces index outside the {nv} vertices")
    frec = _records(TRIANGLES, nf, [], 3)
    frec["vertex_indices.n"], frec["vertex_indices"] = 3, faces
    _write(path, [("vertex", nv, XYZ + RGB), ("face", nf, TRIANGLES)],
           [_records(XYZ + RGB, nv, [("xyz", vertices), (("red", "green", "blue"), colors)]), frec])


def read_mesh_ply(path: str):
    """A file of :func:`write_mesh_ply` -> (vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3]).  ValueError for
    anything else: another layout, a header that is not byte for byte the writer's (a comment line), a truncated body, a
    face that is not a triangle."""
    with open(path, "rb") as f:
        fmt, elements = read_header(f, path)
        end = f.tell()
        f.seek(0)
        if [(e[0], e[2]) for e in elements] != [("vertex", XYZ + RGB), ("face", TRIANGLES)] or f.read(end) != header_bytes(elements):
            raise ValueError(f"{path}: not the layout that write_mesh_ply produces")
        (_, nv, _), (_, nf, _) = elements
        vrec = _read_records(f, path, XYZ + RGB, nv)
        frec = _read_records(f, path, TRIANGLES, nf, 3)
    if nf and not (frec["vertex_indices.n"] == 3).all():
        raise ValueError(f"{path}: faces that are not triangles")
    return _columns(vrec, "xyz"), _columns(vrec, ("red", "green", "blue")), np.ascontiguousarray(frec["vertex_indices"]).reshape(nf, 3)


# ------------------------------------------------------------------------------------------------------------ any file
def read_ply_points(path: str) -> np.ndarray:
    """x, y, z of the ``vertex`` element of a PLY file as float32 [N,3]: ascii, binary_little_endian or binary_big_endian,
    any scalar vertex properties (x, y, z picked by name), other elements before or after it skipped (what plyread.m
    reads at BaseEvalMain_web.m:47-48 and PointCompareMain.m:12-13)."""
    with open(path, "rb") as f:
        fmt, elements = read_header(f, path)
        if "vertex" not in [e[0] for e in elements]:
            raise ValueError(f"{path}: no vertex element")
        end = _FORMATS[fmt]
        for name, count, props in elements:
            if name != "vertex":
                _skip_element(f, end, count, props)
                continue
            pnames = [p[0] for p in props]
            for c in "xyz":
                if c not in pnames:
                    raise ValueError(f"{path}: vertex element has no property {c}")
            if any(isinstance(p[1], tuple) for p in props):
                raise ValueError(f"{path}: list properties in the vertex element are not supported")
            if end is None:
                rows = [f.readline() for _ in range(count)]
                vals = np.array(b" ".join(rows).split(), dtype=np.float64)
                if vals.size != count * len(props):
                    raise ValueError(f"{path}: truncated ascii vertex data")
                vals = vals.reshape(count, len(props))
                return np.stack([vals[:, pnames.index(c)] for c in "xyz"], 1).astype(np.float32)
            dt = _dtype(props, end)
            raw = f.read(dt.itemsize * count)
            if len(raw) != dt.itemsize * count:
                raise ValueError(f"{path}: truncated binary vertex data")
            rec = np.frombuffer(raw, dtype=dt, count=count)
            return np.stack([rec[c].astype(np.float32) for c in "xyz"], 1)
    raise AssertionError("unreachable")


def _skip_element(f, end: Optional[str], count: int, props) -> None:
    """Move ``f`` past an element; ``end``: the byte order, None for ascii."""
    if end is None:
        for _ in range(count):
            f.readline()
        return
    if not any(isinstance(p[1], tuple) for p in props):
        f.seek(_dtype(props, end).itemsize * count, 1)
        return
    for _ in range(count):
        for _, t in props:
            if isinstance(t, tuple):
                cdt = np.dtype(end + t[0])
                k = int(np.frombuffer(f.read(cdt.itemsize), cdt)[0])
                f.seek(k * np.dtype(t[1]).itemsize, 1)
            else:
                f.seek(np.dtype(t).itemsize, 1)
