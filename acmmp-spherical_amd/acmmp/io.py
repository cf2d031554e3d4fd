"""The reference's on-disk formats, OpenCV-free.

  * ReadCamera            ACMMP.cpp:146-209  (cams/%08d_cam.txt; SPHERE and PINHOLE, quirks kept)
  * readDepthDmb/writeDepthDmb, readNormalDmb/writeNormalDmb  ACMMP.cpp:363-479
  * GenerateSampleList    main.cpp:4-33      (pair.txt; sources with score <= 0 dropped)
  * ComputeMultiScaleSettings main.cpp:35-71 (cap 3200, halve until <= 1000)
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np

from .types import PINHOLE, SPHERE, make_camera


def read_camera(path: str) -> np.ndarray:
    """ReadCamera (ACMMP.cpp:146-209).

    Keeps the reference's behaviour: 'extrinsic' + 3 rows of `R|t` + the `0 0 0 1` row,
    'intrinsic' then either `SPHERE f cx cy` or a 3x3 K; then the depth line.  For SPHERE
    all four depth tokens are read as (min, interval, n, max).  For PINHOLE the reader
    stores the 2nd token as depth_max (ACMMP.cpp:205) -- with the converter's
    `d0 dint N dmax` layout (colmap2mvsnet_acm.py:387-388) that is the interval.
    A missing file returns a zeroed camera, as the reference returns its uninitialised one.
    """
    if not os.path.exists(path):
        return make_camera(PINHOLE)
    tok = open(path).read().split()
    it = iter(tok)
    next(it)                                   # "extrinsic"
    R = np.zeros(9, np.float32)
    t = np.zeros(3, np.float32)
    for i in range(3):
        R[3 * i + 0] = float(next(it)); R[3 * i + 1] = float(next(it)); R[3 * i + 2] = float(next(it))
        t[i] = float(next(it))
    for _ in range(4):
        next(it)                               # 0 0 0 1
    next(it)                                   # "intrinsic"
    head = next(it)
    if head == "SPHERE":
        f, cx, cy = float(next(it)), float(next(it)), float(next(it))
        dmin = float(next(it)); float(next(it)); int(float(next(it))); dmax = float(next(it))
        return make_camera(SPHERE, params=[f, cx, cy], R=R, t=t, depth_min=dmin, depth_max=dmax)
    K = np.zeros(9, np.float32)
    K[0] = float(head)
    for k in range(1, 9):
        K[k] = float(next(it))
    dmin, dmax = float(next(it)), float(next(it))
    return make_camera(PINHOLE, K=K, R=R, t=t, depth_min=dmin, depth_max=dmax)


def write_camera(path: str, cam: np.ndarray, depth_interval: float = 0.0, n_planes: int = 192) -> None:
    """Writer matching what colmap2mvsnet_acm.py emits (synthetic scenes; tests)."""
    R = np.asarray(cam["R"]).reshape(3, 3)
    t = np.asarray(cam["t"])
    lines = ["extrinsic"]
    for i in range(3):
        lines.append(" ".join(repr(float(v)) for v in (*R[i], t[i])))
    lines.append("0.0 0.0 0.0 1.0")
    lines.append("")
    lines.append("intrinsic")
    if int(cam["model"]) == SPHERE:
        p = cam["params"]
        lines.append(f"SPHERE {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}")
    else:
        K = np.asarray(cam["K"]).reshape(3, 3)
        for i in range(3):
            lines.append(" ".join(repr(float(v)) for v in K[i]))
    lines.append("")
    lines.append(f"{float(cam['depth_min'])!r} {depth_interval!r} {n_planes} {float(cam['depth_max'])!r}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_dmb(path: str):
    """readDepthDmb / readNormalDmb (ACMMP.cpp:363-452): int32 type(=1), h, w, nb, then h*w*nb floats.

    Returns (h, w) or (h, w, nb) float32, or None where the reference returns -1."""
    try:
        with open(path, "rb") as f:
            hdr = np.fromfile(f, dtype="<i4", count=4)
            if hdr.size < 4 or hdr[0] != 1:
                return None
            _, h, w, nb = (int(v) for v in hdr)
            data = np.fromfile(f, dtype="<f4", count=h * w * nb)
    except OSError:
        return None
    out = np.zeros(h * w * nb, np.float32)
    out[:data.size] = data
    return out.reshape(h, w) if nb == 1 else out.reshape(h, w, nb)


def write_dmb(path: str, arr: np.ndarray) -> None:
    """writeDepthDmb / writeNormalDmb (ACMMP.cpp:395-479)."""
    a = np.ascontiguousarray(arr, np.float32)
    h, w = a.shape[:2]
    nb = 1 if a.ndim == 2 else a.shape[2]
    with open(path, "wb") as f:
        np.array([1, h, w, nb], "<i4").tofile(f)
        a.astype("<f4").tofile(f)


@dataclass
class Problem:
    """struct Problem, main.h:207-213."""
    ref_image_id: int
    src_image_ids: list = field(default_factory=list)
    max_image_size: int = 3200
    num_downscale: int = 0
    cur_image_size: int = 3200


def read_pair_list(dense_folder: str) -> list:
    """GenerateSampleList (main.cpp:4-33)."""
    tok = open(os.path.join(dense_folder, "pair.txt")).read().split()
    it = iter(tok)
    n = int(next(it))
    problems = []
    for _ in range(n):
        p = Problem(int(next(it)))
        m = int(next(it))
        for _ in range(m):
            vid, score = int(next(it)), float(next(it))
            if score <= 0.0:
                continue
            p.src_image_ids.append(vid)
        problems.append(p)
    return problems


def write_pair_list(dense_folder: str, pairs: list) -> None:
    """pairs: list of (ref_id, [(src_id, score), ...])."""
    lines = [str(len(pairs))]
    for ref, srcs in pairs:
        lines.append(str(ref))
        lines.append(" ".join([str(len(srcs))] + [f"{s} {sc!r}" for s, sc in srcs]))
    with open(os.path.join(dense_folder, "pair.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def compute_multiscale_settings(problems: list, image_sizes: dict, max_image_size: int = 3200,
                                size_bound: int = 1000) -> int:
    """ComputeMultiScaleSettings (main.cpp:35-71); image_sizes[ref_id] = (rows, cols)."""
    max_num_downscale = -1
    for p in problems:
        rows, cols = image_sizes[p.ref_image_id]
        max_size = min(max(rows, cols), max_image_size)
        p.max_image_size = max_size
        k = 0
        while max_size > size_bound:
            max_size //= 2
            k += 1
        max_num_downscale = max(max_num_downscale, k)
        p.num_downscale = k
    return max_num_downscale


def scale_schedule(problems: list, max_num_downscale: int) -> list:
    """The per-scale cur_image_size sequence of main.cpp:417-425 (pure; for tests and the driver)."""
    import copy
    ps = copy.deepcopy(problems)
    out = []
    scale = max_num_downscale
    while scale >= 0:
        for p in ps:
            if p.num_downscale >= 0:
                p.cur_image_size = int(p.max_image_size / (2 ** p.num_downscale))
                p.num_downscale -= 1
        out.append([p.cur_image_size for p in ps])
        scale -= 1
    return out


_PLY_RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                        ("r", "u1"), ("g", "u1"), ("b", "u1")])


def _ply_records(points: np.ndarray) -> np.ndarray:
    """(n, 9) float32 fused points -> the PLY's vertex records (the per-vertex rules of write_ply)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 9)
    n = p.shape[0]
    X = p[:, 0:3].copy()
    fmax = np.float32(np.finfo(np.float32).max)
    bad = ~((X[:, 0] < fmax) & (X[:, 0] > -fmax)) | ~((X[:, 1] < fmax) & (X[:, 1] > -fmax)) | \
        ~((X[:, 2] < fmax) & (X[:, 2] >= -fmax))
    X[bad] = 0.0
    rec = np.zeros(n, dtype=_PLY_RECORD)
    rec["x"], rec["y"], rec["z"] = X[:, 0], X[:, 1], X[:, 2]
    rec["nx"], rec["ny"], rec["nz"] = p[:, 3], p[:, 4], p[:, 5]

    def to_char(v):   # (char)(int)v: truncation toward zero, then the low byte
        with np.errstate(invalid="ignore"):
            iv = np.where(np.isfinite(v), np.trunc(v), 0).astype(np.int64)
        return (iv & 0xFF).astype(np.uint8)
    rec["r"], rec["g"], rec["b"] = to_char(p[:, 8]), to_char(p[:, 7]), to_char(p[:, 6])
    return rec


class PlyWriter:
    """write_ply in pieces: the header with the vertex count known up front, then the points in any
    number of write() calls, so a cloud never has to exist as one array.  The bytes are write_ply's.
    close() (or leaving the `with` block without an exception) checks that exactly n_points were written."""

    def __init__(self, path: str, n_points: int):
        self.n, self.written = int(n_points), 0
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {self.n}\n"
                  "property float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        self.f = open(path, "wb")
        self.f.write(header.encode("ascii"))

    def write(self, points: np.ndarray) -> None:
        rec = _ply_records(points)
        if self.written + rec.shape[0] > self.n:
            raise ValueError(f"more than the {self.n} points the header announced")
        self.f.write(rec.tobytes())
        self.written += rec.shape[0]

    def close(self) -> None:
        if self.f is None:
            return
        self.f.close()
        self.f = None
        if self.written != self.n:
            raise ValueError(f"{self.written} points written, the header announced {self.n}")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self.f is not None:
            self.f.close()
            self.f = None
        return False


def write_ply(path: str, points: np.ndarray) -> None:
    """StoreColorPlyFileBinaryPointCloud (ACMMP.cpp:481-534).  points: (n, 9) float32 rows
    x y z nx ny nz c0 c1 c2 as SimpleFusionKernel stores them (c0 = the texture's .z channel);
    the writer emits red = (char)(int)c2, green = (char)(int)c1, blue = (char)(int)c0 and zeroes
    coordinates that are not finite (the FLT_MAX tests of :508-512, including the z >= -FLT_MAX quirk)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 9)
    with PlyWriter(path, p.shape[0]) as w:
        w.write(p)


def read_ply(path: str) -> np.ndarray:
    """Reader for write_ply's layout (tests): structured array x y z nx ny nz r g b."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int([l for l in data[:end].decode().splitlines() if l.startswith("element vertex")][0].split()[2])
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("r", "u1"), ("g", "u1"), ("b", "u1")])
    return np.frombuffer(data[end:end + n * dt.itemsize], dtype=dt).copy()


_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


class MeshPlyWriter:
    """A triangle mesh as a binary PLY in pieces: write_ply's vertex records, then `element face` with
    `property list uchar int vertex_indices`.  The counts are known up front; the vertices come in any number of
    write_vertices() calls, then the faces in any number of write_faces() calls.  close() (or leaving the `with`
    block without an exception) checks that exactly the announced numbers were written."""

    def __init__(self, path: str, n_vertices: int, n_faces: int):
        self.nv, self.nf, self.wv, self.wf = int(n_vertices), int(n_faces), 0, 0
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {self.nv}\n"
                  "property float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  f"element face {self.nf}\n"
                  "property list uchar int vertex_indices\nend_header\n")
        self.f = open(path, "wb")
        self.f.write(header.encode("ascii"))

    def write_vertices(self, vertices: np.ndarray) -> None:
        rec = _ply_records(vertices)
        if self.wf:
            raise ValueError("vertices after the first face")
        if self.wv + rec.shape[0] > self.nv:
            raise ValueError(f"more than the {self.nv} vertices the header announced")
        self.f.write(rec.tobytes())
        self.wv += rec.shape[0]

    def write_faces(self, faces: np.ndarray) -> None:
        t = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        if self.wv != self.nv:
            raise ValueError(f"faces after {self.wv} of {self.nv} vertices")
        if self.wf + t.shape[0] > self.nf:
            raise ValueError(f"more than the {self.nf} faces the header announced")
        if t.size and (t.min() < 0 or t.max() >= self.nv):
            raise ValueError("a face index outside the vertices")
        rec = np.zeros(t.shape[0], _PLY_FACE)
        rec["n"], rec["v"] = 3, t
        self.f.write(rec.tobytes())
        self.wf += t.shape[0]

    def close(self) -> None:
        if self.f is None:
            return
        self.f.close()
        self.f = None
        if self.wv != self.nv or self.wf != self.nf:
            raise ValueError(f"{self.wv} vertices and {self.wf} faces written, the header announced {self.nv} and {self.nf}")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self.f is not None:
            self.f.close()
            self.f = None
        return False


def write_mesh_ply(path: str, vertices: np.ndarray, faces: np.ndarray) -> None:
    """vertices: (n, 9) float32 rows as write_ply's points; faces: (m, 3) int32 vertex indices."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 9)
    t = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    with MeshPlyWriter(path, v.shape[0], t.shape[0]) as w:
        w.write_vertices(v)
        w.write_faces(t)


def read_mesh_ply(path: str):
    """Reader for write_mesh_ply's layout (tests): (read_ply's structured vertex array, faces (m, 3) int32)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().splitlines()
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[2])
    verts = np.frombuffer(data[end:end + nv * _PLY_RECORD.itemsize], dtype=_PLY_RECORD).copy()
    at = end + nv * _PLY_RECORD.itemsize
    rec = np.frombuffer(data[at:at + nf * _PLY_FACE.itemsize], dtype=_PLY_FACE)
    if len(data) != at + nf * _PLY_FACE.itemsize or (rec["n"] != 3).any():
        raise ValueError("not a triangle mesh of write_mesh_ply's layout")
    return verts, rec["v"].astype(np.int32)


@dataclass
class Region:
    """An evaluation region (acmmp_fusion_set_region, include/acmmp.h): the intersection of the parts that are not None.
    planes (k, 4) float64 half-spaces a x + b y + c z + d >= 0; prism: axis w, [axis_min, axis_max] along it and polygon
    (n, 2) float64 in the other two coordinates in increasing index order; grid: origin (3,), cell, dims (nx, ny, nz) and
    bits, ceil(nx ny nz / 8) bytes, cell (ix, iy, iz) at bit k & 7 (least significant first) of byte k >> 3 with
    k = ix + nx (iy + ny iz)."""
    planes: np.ndarray | None = None
    axis: int = 0
    axis_min: float = 0.0
    axis_max: float = 0.0
    polygon: np.ndarray | None = None
    origin: np.ndarray | None = None
    cell: float = 0.0
    dims: tuple | None = None
    bits: np.ndarray | None = None


def read_region(path: str) -> Region:
    """An evaluation region from a JSON file of either kind:
    an Open3D SelectionPolygonVolume as Tanks and Temples ships its crop files ("class_name", "orthogonal_axis" "X", "Y"
    or "Z", "axis_min", "axis_max", "bounding_polygon" of xyz triples, of which the two coordinates other than the axis are
    taken, in increasing index order); or the project's own {"planes": [[a, b, c, d], ...], "prism": {"axis": 0|1|2, "min":,
    "max":, "polygon": [[u, v], ...]}, "grid": {"origin": [x, y, z], "cell":, "dims": [nx, ny, nz], "bits": "file.bin"}},
    every part optional, the bits file relative to the JSON.  The bits file is the grid packed eight cells to a byte, least
    significant bit first, x fastest.  There is no .mat reader: a DTU ObsMask(ix, iy, iz) is exported in MATLAB's own
    column-major order, ObsMask(:), which is already x fastest -- pad it with zeros to a multiple of 8 and pack each run of
    8 cells into one byte, the first cell in bit 0; from numpy that is np.packbits(mask.ravel(order="F"),
    bitorder="little") for mask[ix, iy, iz].  The origin is the centre of cell (0, 0, 0) (DTU: BB(1, :)) and cell the
    grid's resolution, since a point's cell is rint((p - origin) / cell)."""
    import json
    with open(path) as f:
        d = json.load(f)
    r = Region()
    if "class_name" in d:
        if d["class_name"] != "SelectionPolygonVolume":
            raise ValueError(f"{path}: class_name {d['class_name']!r} is not SelectionPolygonVolume")
        axis = {"X": 0, "Y": 1, "Z": 2}.get(str(d["orthogonal_axis"]).upper())
        if axis is None:
            raise ValueError(f"{path}: orthogonal_axis must be X, Y or Z")
        poly = np.asarray(d["bounding_polygon"], np.float64).reshape(-1, 3)
        r.axis, r.axis_min, r.axis_max = axis, float(d["axis_min"]), float(d["axis_max"])
        r.polygon = np.ascontiguousarray(poly[:, [k for k in range(3) if k != axis]])
        return r
    unknown = set(d) - {"planes", "prism", "grid"}
    if unknown:
        raise ValueError(f"{path}: unknown keys {sorted(unknown)}")
    if d.get("planes"):
        r.planes = np.ascontiguousarray(np.asarray(d["planes"], np.float64).reshape(-1, 4))
    if "prism" in d:
        p = d["prism"]
        r.axis, r.axis_min, r.axis_max = int(p["axis"]), float(p["min"]), float(p["max"])
        r.polygon = np.ascontiguousarray(np.asarray(p["polygon"], np.float64).reshape(-1, 2))
    if "grid" in d:
        g = d["grid"]
        r.origin = np.asarray(g["origin"], np.float64).reshape(3)
        r.cell = float(g["cell"])
        r.dims = tuple(int(x) for x in g["dims"])
        if len(r.dims) != 3 or min(r.dims) < 1:
            raise ValueError(f"{path}: dims must be three positive integers")
        r.bits = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(path)), g["bits"]), np.uint8)
        need = (r.dims[0] * r.dims[1] * r.dims[2] + 7) // 8
        if r.bits.size != need:
            raise ValueError(f"{path}: the bits file holds {r.bits.size} bytes, the grid needs {need}")
    return r
