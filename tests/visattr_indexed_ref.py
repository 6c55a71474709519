"""ctypes loader of tests/visattr_indexed_ref.c, the CPU restatement of nv_visibility_attributes_indexed (test infrastructure).

`load(directory)` compiles it there twice, as tests/visattr_ref.py does its parent: fp32 (the bits the kernel must write) and -DREAL=double.
IndexedAttrRef.attributes returns AttrRef.attributes' dict."""
import ctypes as C
import os
import subprocess

import numpy as np

import raster_ref as RR
from niagara_amd import layouts as L
from visattr_ref import _SLICES, VALS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "visattr_indexed_ref.c")


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class IndexedAttrRef:
    def __init__(self, so32, so64):
        self.libs = {"f32": C.CDLL(so32), "f64": C.CDLL(so64)}
        for k, size in (("f32", 4), ("f64", 8)):
            self.libs[k].vai_attributes.restype = None
            assert self.libs[k].va_real_bytes() == size

    def attributes(self, g, records, width, height, draws, indices, vertices, materials=None, real="f32", counts=None):
        """AttrRef.attributes over layouts.VISINDEXEDRECORD records; counts: {"draws" / "indices" / "vertices" / "materials": n} overrides a
        capacity"""
        rt = np.float32 if real == "f32" else np.float64
        n = width * height
        records = np.ascontiguousarray(records, L.VISINDEXEDRECORD).reshape(-1)
        assert len(records) == n
        draws, indices = np.ascontiguousarray(draws, L.MESHDRAW), np.ascontiguousarray(indices, np.uint32)
        vertices = np.ascontiguousarray(vertices, L.VERTEX)
        mats = None if materials is None else np.ascontiguousarray(materials, L.MATERIAL)
        cnt = dict(draws=len(draws), indices=len(indices), vertices=len(vertices), materials=0 if mats is None else len(mats))
        cnt.update(counts or {})
        out = dict(vals=np.zeros((n, 14), rt), ids=np.zeros((n, 2), np.uint32), gbuffer0=np.zeros(n, np.uint32), gbuffer1=np.zeros(n, np.uint32),
                   totals=np.zeros(4, np.uint64), flags=np.zeros(n, np.uint8), chan=np.zeros((n, 8), rt))
        one = lambda a, dt: a if len(a) else np.zeros(1, dt)
        self.libs[real].vai_attributes(_p(np.ascontiguousarray(g)), _p(records), C.c_uint32(width), C.c_uint32(height), _p(one(draws, L.MESHDRAW)),
                                       C.c_uint32(cnt["draws"]), _p(one(indices, np.uint32)), C.c_uint32(cnt["indices"]),
                                       _p(one(vertices, L.VERTEX)), C.c_uint32(cnt["vertices"]), _p(mats), C.c_uint32(cnt["materials"]),
                                       _p(out["vals"]), _p(out["ids"]), _p(out["gbuffer0"]), _p(out["gbuffer1"]), _p(out["totals"]),
                                       _p(out["flags"]), _p(out["chan"]))
        for name, sl in _SLICES.items():
            out[name] = out["vals"][:, sl]
        if real == "f32":
            a = np.zeros(n, L.PIXELATTR)
            for name in VALS:
                a[name] = out[name]
            a["drawId"], a["materialIndex"] = out["ids"][:, 0], out["ids"][:, 1]
            out["attributes"] = a
        return out


def load(directory):
    so32, so64 = (os.path.join(str(directory), "libvisattr_indexed_ref_%s.so" % k) for k in ("f32", "f64"))
    for so, extra in ((so32, []), (so64, ["-DREAL=double"])):
        if not os.path.exists(so):
            subprocess.check_call(["gcc"] + RR.FLAGS + extra + ["-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", HERE, "-o", so, SRC, "-lm"])
    return IndexedAttrRef(so32, so64)
