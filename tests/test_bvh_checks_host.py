"""The shared tree checkers of tests/bvh_checks.py, checked themselves where no device is needed: padded_boxes against the host builder's
leaf boxes (the same formula, compiled from csrc/bvh_build.cpp), the device-tree checker on a tree put together here - it passes the
correct tree and sees every defect it exists for -, cost8 on known trees, and the case generator's counts."""
import ctypes as C

import numpy as np
import pytest

import bvh_checks as BC
from adapt_amd import _lib

F32 = np.float32


def _host_tree(fs):
    lib = _lib.load()
    prims, info = np.ascontiguousarray(fs.prims, F32), np.ascontiguousarray(fs.obj_info, np.int32)
    h = C.c_void_p()
    _lib.check(lib.apt_bvh_build(prims.ctypes.data_as(_lib.f32p), fs.n_prims, info.ctypes.data_as(_lib.i32p), fs.n_objects, C.byref(h)))
    try:
        nn, npr, dep, wn, lv = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(lib.apt_bvh_counts(h, C.byref(nn), C.byref(npr), C.byref(dep)))
        nodes, order = np.zeros((nn.value, 16), F32), np.zeros(npr.value, np.int32)
        _lib.check(lib.apt_bvh_export(h, nodes.ctypes.data_as(_lib.f32p), order.ctypes.data_as(_lib.i32p)))
        _lib.check(lib.apt_bvh_wide_counts(h, C.byref(wn), C.byref(lv)))
        wide, worder = np.zeros((wn.value, 16), np.uint32), np.zeros(fs.n_prims, np.int32)
        _lib.check(lib.apt_bvh_wide_export(h, wide.ctypes.data_as(_lib.u32p), worder.ctypes.data_as(_lib.i32p)))
        gmin, gstep = np.zeros(3, F32), np.zeros(3, F32)
        _lib.check(lib.apt_bvh_wide_frame(h, gmin.ctypes.data_as(_lib.f32p), gstep.ctypes.data_as(_lib.f32p)))
    finally:
        lib.apt_bvh_free(h)
    return nodes, order, dep.value, wide, worder, lv.value, (gmin, gstep)


def test_the_case_generator_gives_what_its_table_says():
    for n in BC.SOUP_SIZES:
        fs = BC.case(f"soup-{n}")
        assert fs.n_prims == n and fs.prims.shape == (n, 3, 3) and fs.prims.dtype == F32 and np.abs(fs.prims).max() <= 3.0
        assert n < 16 or (fs.prims.min() < -1 and fs.prims.max() > 1)
        assert np.array_equal(fs.obj_info, [[0, n, 0]]) and fs.n_objects == 1
    m = BC.case("mixed")
    sph = BC.sphere_flags(m)
    assert m.n_prims == 800 and sph.sum() == 200 and m.n_objects == 201 and not sph[:600].any()
    r = m.prims[sph, 1, 0]
    assert 1e-3 <= r.min() and r.max() <= 0.5 and (m.prims[sph, 1] == r[:, None]).all() and not m.prims[sph, 2].any()
    assert len(np.unique(m.prims[780:790, 0], axis=0)) == 1 and len(np.unique(r[180:190])) == 10                 # concentric
    assert len(np.unique(m.prims[790:800].reshape(10, -1), axis=0)) == 1                                          # identical
    p = BC.case("planar")
    assert p.n_prims == 2048 and (p.prims[:, :, 1] == 0.5).all()
    c = BC.case("coincident")
    assert c.n_prims == 301 and len(np.unique(c.prims.reshape(301, -1), axis=0)) == 2
    rb = BC.case("ribbon")
    assert rb.n_prims == 5000 and np.array_equal(rb.prims[1:] - rb.prims[:-1], np.broadcast_to(F32([0.125, 0, 0]), (4999, 3, 3)))
    o = BC.case("outlier")
    assert o.n_prims == 1001 and np.array_equal(o.prims[:1000], BC.case("soup-1000").prims) and o.prims[1000, :, 0].min() == 1e4
    b, bc = BC.case("bunnies1"), BC.case("bunnies1-centred")
    assert b.n_prims == bc.n_prims == 5950 and b.prims.min() >= 0 and bc.prims.min() < -2 and bc.prims.max() > 2
    assert BC.case("mixed") is m and np.array_equal(BC._soup(600, 8), m.prims[:600])                                # seeded


@pytest.mark.parametrize("name", ["mixed", "soup-257", "bunnies1-centred", "outlier"])
def test_padded_boxes_are_the_host_builders_leaf_boxes(name):
    """The host builder pads with the formula the device builder copies.  Every leaf box of its exported tree (up to four primitives) is,
    bit for bit, the min / max over padded_boxes of the leaf's primitives: triangles and spheres, both signs, a coordinate of 1e4."""
    fs = BC.case(name)
    nodes, order, _, *_ = _host_tree(fs)
    pb = BC.padded_boxes(fs)
    assert pb.dtype == F32 and pb.shape == (fs.n_prims, 6)
    links = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32)
    boxes = nodes[:, :12].reshape(-1, 2, 6)
    n_leaves = 0
    for k, c in zip(*np.nonzero(links < 0)):
        code = ~int(links[k, c])
        p = pb[order[(code >> 4):(code >> 4) + (code & 15)]]
        want = np.concatenate([p[:, :3].min(axis=0), p[:, 3:].max(axis=0)])
        assert np.array_equal(boxes[k, c].view(np.uint32), want.view(np.uint32)), (k, c)
        n_leaves += code & 15
    assert n_leaves == fs.n_prims


def _median_tree(fs):
    """a correct tree with the radix-tree property, put together in numpy: primitives sorted along x, ranges halved, preorder node numbers"""
    pb = BC.padded_boxes(fs)
    order = np.argsort(fs.prims[:, :, 0].sum(axis=1), kind="stable").astype(np.int32)
    n = fs.n_prims
    nodes = np.zeros((n - 1, 16), F32)
    links = np.zeros((n - 1, 2), np.int32)
    count, depth = [0], [0]

    def build(a, b, d):
        if b - a == 1:
            depth[0] = max(depth[0], d)
            return ~((a << 4) | 1), pb[order[a]]
        me = count[0]; count[0] += 1
        mid = (a + b + 1) // 2
        box = []
        for c, (x, y) in enumerate(((a, mid), (mid, b))):
            links[me, c], bx = build(x, y, d + 1)
            nodes[me, 6 * c:6 * c + 6] = bx
            box.append(bx)
        return me, np.concatenate([np.minimum(box[0][:3], box[1][:3]), np.maximum(box[0][3:], box[1][3:])])

    build(0, n, 0)
    nodes[:, 12:14] = links.view(F32)
    return nodes, order, depth[0]


def test_the_device_tree_checker_passes_a_correct_tree_and_sees_each_defect():
    fs = BC.case("soup-65")
    nodes, order, depth = _median_tree(fs)
    BC.check_device_binary_tree(fs, nodes, order, depth, radix=True)
    links = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32)
    inner = np.argwhere(links >= 0)
    leaf = np.argwhere(links < 0)

    def broken(change, radix=False, match=None):
        bad, bad_order = nodes.copy(), order.copy()
        new_depth = change(bad, bad_order)
        with pytest.raises(AssertionError, match=match):
            BC.check_device_binary_tree(fs, bad, bad_order, depth if new_depth is None else new_depth, radix=radix)

    k, c = inner[5]

    def too_large(bad, _):            # a box left one ulp too large: what a fit that read a sibling too early, or never shrank, leaves
        bad[k, 6 * c + 3] = np.nextafter(bad[k, 6 * c + 3], F32(np.inf))
    broken(too_large, match="inner boxes are not the union")

    def too_small(bad, _):
        bad[k, 6 * c] = np.nextafter(bad[k, 6 * c], F32(np.inf))
    broken(too_small, match="inner boxes are not the union")
    lk, lc = leaf[7]

    def leaf_box(bad, _):
        bad[lk, 6 * lc + 1] = np.nextafter(bad[lk, 6 * lc + 1], F32(-np.inf))
    broken(leaf_box, match="leaf boxes differ")

    def lost_primitive(bad, _):       # two leaf links to one slot
        bad[leaf[1][0], 12 + leaf[1][1]] = bad[leaf[0][0], 12 + leaf[0][1]]
    broken(lost_primitive, match="hangs in the tree twice")

    def shared_node(bad, _):          # a node reached twice, another never
        bad[inner[3][0], 12 + inner[3][1]] = bad[inner[9][0], 12 + inner[9][1]]
    broken(shared_node, match="reached twice")

    def four_per_leaf(bad, _):
        v = bad[lk, 12 + lc:13 + lc].view(np.int32); v[0] = ~((~v[0]) | 4)
    broken(four_per_leaf, match="exactly one primitive")

    def not_a_permutation(_, bad_order):
        bad_order[3] = bad_order[4]
    broken(not_a_permutation, match="not a permutation")
    broken(lambda *_: 64, match=None)                                    # the hard-coded depth of the scene path is not the tree's

    def swapped_children(bad, _):     # still a correct tree, no longer a radix tree
        bad[k] = np.concatenate([bad[k, 6:12], bad[k, 0:6], bad[k, 13:14], bad[k, 12:13], bad[k, 14:16]])
    bad = nodes.copy(); swapped_children(bad, None)
    BC.check_device_binary_tree(fs, bad, order, depth, radix=False)
    broken(swapped_children, radix=True, match="do not lie before")


def test_cost8_counts_child_box_areas():
    """A root with eight equal children that tile it: each child box has a quarter of the root's half area -> cost 8 / 4 = 2, whatever the
    grid steps; on a real tree the figure is above that, and it grows when the tree gets worse (boxes stretched)."""
    node = np.zeros((1, 16), np.uint32)
    node[0, 1] = 0xff << 16                                             # eight leaf slots, corner 0, exponents 0
    qlo = np.uint8([[0, 0, 0, 0, 100, 100, 100, 100], [0, 0, 100, 100, 0, 0, 100, 100], [0, 100, 0, 100, 0, 100, 0, 100]])
    node[0, 4:16] = np.concatenate([qlo, qlo + 100]).reshape(-1).view(np.uint32)
    assert BC.cost8(node, (np.zeros(3, F32), np.ones(3, F32))) == pytest.approx(2.0)
    assert BC.cost8(node, (np.zeros(3, F32), F32([0.5, 2, 4]))) == pytest.approx(8 * (0.5 * 2 + 2 * 4 + 0.5 * 4) / (4 * (0.5 * 2 + 2 * 4 + 0.5 * 4)))
    fs = BC.case("soup-1000")
    _, _, _, wide, worder, levels, frame = _host_tree(fs)
    BC.check_wide_tree(fs, wide, worder, levels, frame)
    good = BC.cost8(wide, frame)
    worse = wide.copy()
    by = worse[1:, 4:16].view(np.uint8).reshape(-1, 6, 8)               # every box below the root's node stretched to its node's whole frame
    used = BC.decode_wide(wide)[2][1:] | BC.decode_wide(wide)[3][1:]
    for s in range(8):
        on = ((used >> s) & 1).astype(bool)
        by[on, 0:3, s], by[on, 3:6, s] = 0, 255
    assert 2.0 < good < BC.cost8(worse, frame)
