"""The evaluation-region entry points: declared in include/acmmp.h, exported by the library, listed in capi.EXPORTS; the
struct's layout is the header's; the Python wrappers refuse bad arguments before they reach the library (no device)."""
import os
import re
import subprocess

import numpy as np
import pytest

import eval_region_support as er
from acmmp import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "acmmp.h")
SYMBOLS = ("acmmp_fusion_set_region", "acmmp_fusion_get_region", "acmmp_fusion_region_classify",
           "acmmp_fusion_region_classes")


def test_declared_exported_and_listed():
    header = open(HEADER).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"acmmp_status\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS, name
        assert re.search(r"\sT\s+" + name + r"\s", exported), name
    consts = {k: int(v) for k, v in re.findall(r"#define\s+ACMMP_REGION_(\w+)\s+(\d+)", header)}
    assert {"data": consts["DATA"], "reference": consts["REFERENCE"]} == capi.REGION_SIDES
    assert consts["QUERIES_ONLY"] == capi.REGION_QUERIES_ONLY and consts["COUNT_WORDS"] == len(capi.REGION_COUNTS) == 6
    assert {k.lower(): consts["CLASS_" + k.upper()] for k in capi.REGION_CLASS_BITS} == capi.REGION_CLASS_BITS
    assert (consts["CLASS_INVALID"], consts["CLASS_PLANES"], consts["CLASS_PRISM"], consts["CLASS_GRID"]) == \
        (er.INVALID, er.PLANES, er.PRISM, er.GRID)
    assert (consts["MAX_PLANES"], consts["MAX_VERTICES"], consts["MAX_DIM"]) == (8, 256, 4096)
    assert capi.REGION_SOURCES == dict(capi.DIST_SOURCES, reference=capi.SURF_QUERIES["reference"])
    assert len(set(capi.REGION_SOURCES.values())) == len(capi.REGION_SOURCES)


def test_struct_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in capi.RegionStruct._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu", sizeof(acmmp_region));\n%s  return 0;\n}\n'
                    % (HEADER, "".join('  printf(" %%zu", offsetof(acmmp_region, %s));\n' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    import ctypes as C
    assert vals == [C.sizeof(capi.RegionStruct)] + [getattr(capi.RegionStruct, f).offset for f in fields]


def test_region_struct_of_a_region():
    st, keep = capi.region_struct(er.region(planes=True, prism=True, grid=True))
    assert (st.n_planes, st.n_vertices, st.axis, tuple(st.dims)) == (8, 9, 2, er.GRID_DIMS)
    assert np.array_equal(np.array(st.planes[:32]).reshape(8, 4), er.PLANE_ROWS) and np.signbit(st.planes[31])
    assert (st.axis_min, st.axis_max, st.cell, tuple(st.origin)) == (er.AXIS_MIN, er.AXIS_MAX, er.GRID_CELL, er.GRID_ORIGIN)
    assert st.polygon == keep[0].ctypes.data and st.bits == keep[1].ctypes.data
    assert np.array_equal(keep[0], er.POLYGON) and np.array_equal(keep[1], er.grid_bits())
    empty, keep = capi.region_struct(er.region())
    assert (empty.n_planes, empty.n_vertices, tuple(empty.dims), empty.polygon, empty.bits, keep) == (0, 0, (0, 0, 0), None, None, [])


def test_wrappers_refuse_bad_arguments_without_a_device():
    fu = capi.Fusion.__new__(capi.Fusion)                                  # no library handle: a call would fail loudly
    fu.L = fu.h = None
    good = er.region(planes=True, prism=True, grid=True)
    with pytest.raises(ValueError):
        fu.set_region("both", good)
    with pytest.raises(ValueError):
        fu.region("cloud")
    for change in (dict(planes=np.zeros((9, 4))), dict(polygon=er.POLYGON[:2]), dict(polygon=np.zeros((257, 2))),
                   dict(dims=(5, 7)), dict(dims=(5, 7, 4097)), dict(dims=(0, 7, 9)), dict(bits=er.grid_bits()[:-1])):
        r = er.region(planes=True, prism=True, grid=True)
        for k, v in change.items():
            setattr(r, k, v)
        with pytest.raises(ValueError):
            fu.set_region("data", r)
    for source in ("cloud", "surface", ""):
        with pytest.raises(ValueError):
            fu.region_classify(source)
    for args in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            fu.region_classes(*args)
    for call in (lambda: fu.set_region("data", good), lambda: fu.set_region("reference", None), lambda: fu.region("data"),
                 lambda: fu.region_classify("reference"), lambda: fu.region_classes(0, 1)):
        with pytest.raises(AttributeError):                                # a good call does reach the library
            call()
