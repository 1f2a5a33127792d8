"""Helpers shared by the tests of the flat sweep's record builder (tests/test_flat_records.py, tests/test_shadow_cull.py,
tests/test_camera_cull.py on the CPU; tests/test_gpu_fast.py on the device).  Not collected by pytest (no `test_` prefix); nothing here
needs a device."""
import ctypes as C

import numpy as np

from adapt_amd import _lib


def flat_records(prims, obj_info):
    lib = _lib.load()
    prims = np.ascontiguousarray(prims, np.float32).reshape(-1, 9); obj_info = np.ascontiguousarray(obj_info, np.int32).reshape(-1, 3)
    counts = np.zeros(7, np.int32); ns, nt = C.c_int32(0), C.c_int32(0)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(lib.apt_flat_records(fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(counts), None, 0, None, 0, C.byref(ns), C.byref(nt)), "apt_flat_records", lib)
    stream, tab = np.zeros(ns.value, np.float32), np.zeros(nt.value, np.float32)
    _lib.check(lib.apt_flat_records(fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(counts), fp(stream), ns.value, fp(tab), nt.value, C.byref(ns), C.byref(nt)), "apt_flat_records", lib)
    return counts, stream, tab


def sections(counts):
    """per record: section (0 parallelogram, 1 convex quad, 2 triangle, 3 sphere) and its offset in the stream"""
    n = [counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]]
    out, at = [], 0
    for sec, w in enumerate((12, 18, 12, 4)):
        for _ in range(n[sec]):
            out.append((sec, at)); at += w
    return out


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _quad_soup(seed):
    """A scene of planar shapes for the flat sweep's record builder (csrc/flat_build.cpp): convex quadrilaterals, parallelograms, concave
    quadrilaterals (their two triangles must NOT be merged into a convex-quad record), slightly folded quads (not coplanar: not merged),
    triangle fans, coplanar triangles that share no edge, lone triangles - every triangle with a random vertex rotation."""
    from adapt_amd import synth
    rs = np.random.RandomState(seed)
    b = synth._Builder()
    white = synth._brdf("lambertian", "#BDBDBD")

    def frame():
        n = rs.normal(size=3); n /= np.linalg.norm(n)
        a = np.cross(n, rs.normal(size=3)); a /= np.linalg.norm(a)
        return rs.uniform(1.0, 4.5, 3), a, np.cross(n, a), n

    def rot(tri):
        k = rs.randint(3)
        return np.roll(tri, k, axis=0)

    def emit(tris):
        b.mesh(np.float32([rot(np.asarray(t)) for t in tris]), white)

    for kind in ["convex"] * 6 + ["para"] * 3 + ["concave"] * 3 + ["folded"] * 2:
        c, a, bb, n = frame()
        if kind == "convex":
            ang = np.sort(rs.uniform(0, 2 * np.pi, 4)); ang += np.float64([0.0, 0.3, 0.6, 0.9])      # four points around a centre, in order
            rad = rs.uniform(0.5, 1.2, 4)
            pts = [c + r * (np.cos(t) * a + np.sin(t) * bb) for r, t in zip(rad, ang)]
            hull_ok = all(np.dot(np.cross(pts[(i + 1) % 4] - pts[i], pts[(i + 2) % 4] - pts[(i + 1) % 4]), n) > 0 for i in range(4))
            if not hull_ok:
                pts = [c + 0.8 * (np.cos(t) * a + np.sin(t) * bb) for t in (0.2, 1.9, 3.3, 4.9)]
        elif kind == "para":
            e1, e2 = rs.uniform(0.5, 1.2) * a + rs.uniform(-0.3, 0.3) * bb, rs.uniform(0.5, 1.2) * bb
            pts = [c, c + e1, c + e1 + e2, c + e2]
        elif kind == "concave":
            pts = [c + 1.0 * a, c + 0.15 * (a + bb), c + 1.0 * bb, c - 0.8 * (a + bb)]                # reflex corner at pts[1]: split along 1-3
            emit([[pts[1], pts[2], pts[3]], [pts[1], pts[3], pts[0]]])
            continue
        else:
            pts = [c, c + a, c + a + bb + 2e-3 * n, c + bb]
        emit([[pts[0], pts[1], pts[2]], [pts[0], pts[2], pts[3]]])
    c, a, bb, n = frame()                                                                            # a fan of five coplanar triangles
    ring = [c + 0.9 * (np.cos(t) * a + np.sin(t) * bb) for t in np.linspace(0, 2 * np.pi, 6)[:-1]]
    emit([[c, ring[i], ring[(i + 1) % 5]] for i in range(5)])
    c, a, bb, n = frame()                                                                            # coplanar, no shared edge
    emit([[c, c + a, c + bb], [c + 1.5 * a, c + 2.5 * a, c + 1.5 * a + bb]])
    emit([[rs.uniform(0.5, 5.0, 3) for _ in range(3)] for _ in range(10)])                           # lone triangles
    em = [synth._spot("6.0, 6.0, 6.0", "100.0", (2.7, 5.0, 2.7), (0.0, -1.0, 0.0), 40.0, "s")]
    return b.finish(em, synth._sensor(64, 64, 4, 1))
