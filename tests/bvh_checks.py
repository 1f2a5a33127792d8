"""Checkers for exported trees, shared by tests/test_abi.py (host SAH builder, 8-wide collapse) and tests/test_gpu_bvh_device.py (the
device builders of csrc/bvh_gpu.hip), and the primitive sets the device builders are tried on.  Not collected.

A scene here is any object with `prims` (n, 3, 3) float32 - triangle v0 v1 v2 | sphere centre, (r, r, r), 0 -, `n_prims`, `obj_info`
(n_objects, 3) int32 - first primitive, count, 1 = sphere - and `n_objects`.

Nothing in this module replays a builder's decisions (Morton keys, radix splits, PLOC merges).  It checks what every correct tree has,
whatever the builder: the links form a tree, every primitive hangs in it once, every box is what lies below it."""
import functools

import numpy as np

F32 = np.float32


def prim_bounds(fs, k, sphere):
    v = fs.prims[k]
    if sphere:
        return v[0] - v[1], v[0] + v[1]
    return v.min(axis=0), v.max(axis=0)


def sphere_flags(fs):
    return np.repeat(fs.obj_info[:, 2], fs.obj_info[:, 1]).astype(bool)


def padded_boxes(fs):
    """(n, 6) float32: the padded primitive boxes of the builders (csrc/bvh_build.cpp, csrc/bvh_gpu.hip k_prim_boxes), their formula in
    their operation order: pad = 1e-4f + 1e-5f * max(|lo|, |hi|), box lo - pad .. hi + pad; a sphere's lo, hi = centre -+ r.  Every
    operation is one float32 rounding here as there (the library is compiled with -ffp-contract=off)."""
    p = np.ascontiguousarray(fs.prims, F32).reshape(-1, 3, 3)
    lo, hi = p.min(axis=1), p.max(axis=1)
    sph = sphere_flags(fs)
    r = p[sph, 1, 0:1]                                     # the builders read the first of (r, r, r) for every axis
    lo[sph], hi[sph] = p[sph, 0] - r, p[sph, 0] + r
    pad = F32(1e-4) + F32(1e-5) * np.maximum(np.abs(lo), np.abs(hi))
    assert pad.dtype == F32
    return np.concatenate([lo - pad, hi + pad], axis=1)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- binary tree, host builder
def check_binary_tree(fs, nodes, order, depth):
    """Own builder (csrc/bvh_build.cpp): every primitive in exactly one leaf, child boxes bound their subtree."""
    assert sorted(order.tolist()) == list(range(fs.n_prims))
    sphere = sphere_flags(fs)
    links = nodes[:, 12:14].copy().view(np.int32)
    seen_nodes, seen_slots = set(), []

    def walk(link, lo, hi, d):
        assert d <= depth + 1
        if link < 0:
            code = ~int(link)
            first, count = code >> 4, code & 15
            assert 0 < count <= 4 or fs.n_prims == 0
            for s in range(first, first + count):
                plo, phi = prim_bounds(fs, order[s], sphere[order[s]])
                assert np.all(plo >= lo) and np.all(phi <= hi)
                seen_slots.append(s)
            return
        assert link not in seen_nodes
        seen_nodes.add(int(link))
        nd = nodes[link]
        for c, (a, b) in enumerate(((0, 3), (6, 9))):
            clo, chi = nd[a:a + 3], nd[b:b + 3]
            if lo is not None:
                assert np.all(clo >= lo - 1e-6) and np.all(chi <= hi + 1e-6)
            walk(int(links[link, c]), clo, chi, d + 1)

    walk(0, None, None, 0)
    assert sorted(seen_slots) == list(range(fs.n_prims)) and len(seen_nodes) == nodes.shape[0]


# ---------------------------------------------------------------------------------------------- binary tree, device builders
def check_device_binary_tree(fs, nodes, order, depth, radix):
    """A device-built binary tree as apt_bvh_export hands it out (16 floats per node: left box, right box, left link, right link; a leaf
    link is ~(slot << 4 | count)).  Depth is the host builder's count: node 0 at 0, a leaf one below its node.

    Every tree: n - 1 nodes, each reached exactly once from node 0; every leaf link holds exactly one primitive; prim_order is a
    permutation and every slot hangs in the tree once; `depth` is the depth the walk finds; every leaf box equals padded_boxes bit for
    bit; every inner child's box equals, bit for bit, the min / max over the two boxes stored in that child.
    radix (LBVH): the leaves under every node are one contiguous range of prim_order, the left child's before the right child's, and
    the depth is at most 64 (62-bit keys).

    The walk keeps its own stack, so a chain-shaped tree is a failed depth check somewhere, not a recursion error here."""
    n = fs.n_prims
    assert nodes.shape == (n - 1, 16) and order.shape == (n,)
    assert np.array_equal(np.sort(order), np.arange(n)), "prim_order is not a permutation"
    links = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32)
    assert not nodes[:, 14:16].any()
    leaf = links < 0
    code = ~links[leaf]
    assert ((code & 15) == 1).all(), "a leaf link that does not hold exactly one primitive"
    assert ((code >> 4) < n).all() and (links[~leaf] < n - 1).all(), "a link out of range"
    # ---- the walk: every node once, preorder, depths
    visits, node_depth, pre = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), []
    stack = [(0, 0)]
    while stack:
        k, d = stack.pop()
        visits[k] += 1
        assert visits[k] == 1, f"node {k} is reached twice"
        node_depth[k] = d
        pre.append(k)
        for c in (1, 0):
            if links[k, c] >= 0:
                stack.append((int(links[k, c]), d + 1))
    assert (visits == 1).all(), f"{int((visits == 0).sum())} nodes are not reached from node 0"
    slots = np.sort(code >> 4)
    assert np.array_equal(slots, np.arange(n)), "a primitive hangs in the tree twice, or not at all"
    walked_depth = int(node_depth[leaf.any(axis=1)].max()) + 1          # the deepest node that carries a leaf, and one below it
    assert depth == walked_depth, (depth, walked_depth)
    # ---- leaf boxes: the padded primitive box, bit for bit
    boxes = nodes[:, :12].reshape(n - 1, 2, 6)
    want = padded_boxes(fs)[order[code >> 4]]
    same = (_bits(boxes[leaf]) == _bits(want)).all(axis=1)
    assert same.all(), f"{int((~same).sum())} leaf boxes differ from the padded primitive box, first at slot {int((code >> 4)[~same][0])}"
    # ---- inner boxes: a child's box, as its parent stores it, is the min / max over the two boxes the child stores
    union = np.concatenate([np.minimum(boxes[:, 0, :3], boxes[:, 1, :3]), np.maximum(boxes[:, 0, 3:], boxes[:, 1, 3:])], axis=1)
    inner = ~leaf
    same = (_bits(boxes[inner]) == _bits(union[links[inner]])).all(axis=1)
    assert same.all(), f"{int((~same).sum())} inner boxes are not the union of the two boxes below them, first: child node {int(links[inner][~same][0])}"
    if not radix:
        return
    # ---- the radix-tree property, bottom up over the preorder
    lo, hi, cnt = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    for k in reversed(pre):
        r = []
        for c in (0, 1):
            L = int(links[k, c])
            r.append((~L >> 4, ~L >> 4, 1) if L < 0 else (lo[L], hi[L], cnt[L]))
        assert r[0][1] < r[1][0], f"node {k}: the left child's leaves do not lie before the right child's"
        lo[k], hi[k], cnt[k] = r[0][0], r[1][1], r[0][2] + r[1][2]
        assert hi[k] - lo[k] + 1 == cnt[k], f"node {k}: its leaves are not one contiguous range of prim_order"
    assert depth <= 64


# ---------------------------------------------------------------------------------------------- the 8-wide tree
def decode_wide(nodes):
    """64-byte nodes (csrc/bvh_wide.cpp) -> per node: corner (3,) in grid units, scale (3,) = 2^e in grid units, leaf mask, inner mask,
    child_base, tri_base, qlo (3, 8), qhi (3, 8)"""
    w = nodes.astype(np.int64)
    corner = np.stack([w[:, 0] & 0xffff, w[:, 0] >> 16, w[:, 1] & 0xffff], 1)
    lmask, imask = (w[:, 1] >> 16) & 0xff, w[:, 1] >> 24
    ex = np.stack([(w[:, 2] >> 24) & 15, w[:, 2] >> 28, (w[:, 3] >> 24) & 15], 1)
    assert ((w[:, 3] >> 28) == 0).all()
    by = np.ascontiguousarray(nodes[:, 4:16]).view(np.uint8).reshape(-1, 6, 8)
    return corner, np.ldexp(1.0, ex), lmask, imask, w[:, 2] & 0xffffff, w[:, 3] & 0xffffff, by[:, 0:3], by[:, 3:6]


def check_wide_tree(fs, nodes, order, levels, frame):
    """Every primitive sits in exactly one leaf child (one primitive per leaf, at most eight per node); inner children are consecutive and
    counted by the inner-slot mask, leaf primitives by the leaf-slot mask; every decoded child box contains the boxes of all primitives
    below it (the quantisation rounds outwards, the 16-bit corner lies at or below the node's box); `levels` is the depth the walk finds."""
    gmin, gstep = frame
    assert sorted(order.tolist()) == list(range(fs.n_prims))
    assert np.all(np.log2(gstep.astype(np.float64)) % 1 == 0)                           # power-of-two steps: the grid transform is exact
    corner, sc, lmask, imask, cbase, tbase, qlo, qhi = decode_wide(nodes)
    assert (corner >= 0).all() and (corner <= 65535).all() and (lmask & imask == 0).all()
    sphere = sphere_flags(fs)
    seen_nodes, seen_slots, depth_seen = set(), [], [0]
    g0, gs = gmin.astype(np.float64), gstep.astype(np.float64)

    def walk(n, d):
        assert n not in seen_nodes and d <= levels
        seen_nodes.add(n); depth_seen[0] = max(depth_seen[0], d)
        lo_all, hi_all = np.full(3, np.inf), np.full(3, -np.inf)
        rank, tri_next = 0, 0
        for s in range(8):
            leaf, inner = bool((lmask[n] >> s) & 1), bool((imask[n] >> s) & 1)
            if not (leaf or inner):
                assert (qlo[n, :, s] == 255).all() and (qhi[n, :, s] == 0).all()          # inverted box: never hit
                continue
            blo = g0 + gs * (corner[n] + qlo[n, :, s].astype(np.float64) * sc[n])            # world = gmin + gstep * (corner + q * 2^e), exact in double
            bhi = g0 + gs * (corner[n] + qhi[n, :, s].astype(np.float64) * sc[n])
            if inner:
                clo, chi = walk(int(cbase[n]) + rank, d + 1)
                rank += 1
            else:
                slot = int(tbase[n]) + tri_next
                a, b = prim_bounds(fs, order[slot], sphere[order[slot]])
                clo, chi = a.astype(np.float64), b.astype(np.float64)
                seen_slots.append(slot)
                tri_next += 1
            assert np.all(blo <= clo) and np.all(bhi >= chi), (n, s)
            lo_all, hi_all = np.minimum(lo_all, clo), np.maximum(hi_all, chi)
        return lo_all, hi_all

    walk(0, 1)
    assert sorted(seen_slots) == list(range(fs.n_prims)) and len(seen_nodes) == nodes.shape[0] and depth_seen[0] == levels


def cost8(nodes, frame):
    """The expected number of child-box hits of a random line through the root box: the sum, over the occupied child slots of all 8-wide
    nodes, of the decoded child box's half area, divided by the root box's half area (the union of the root node's child boxes)."""
    gstep = np.asarray(frame[1], np.float64)
    corner, sc, lmask, imask, _, _, qlo, qhi = decode_wide(nodes)
    used = (((lmask | imask)[:, None] >> np.arange(8)) & 1).astype(bool)                               # (nodes, 8)
    lo = (corner[:, :, None] + qlo.astype(np.float64) * sc[:, :, None]) * gstep[None, :, None]        # (nodes, 3, 8), world units from gmin
    hi = (corner[:, :, None] + qhi.astype(np.float64) * sc[:, :, None]) * gstep[None, :, None]

    def half_area(d):
        return d[..., 0, :] * d[..., 1, :] + d[..., 1, :] * d[..., 2, :] + d[..., 0, :] * d[..., 2, :]

    area = half_area(hi - lo)
    assert (area[used] >= 0).all() and used[0].any()
    root = hi[0][:, used[0]].max(axis=1) - lo[0][:, used[0]].min(axis=1)
    return float(area[used].sum() / half_area(root[:, None])[0])


# ---------------------------------------------------------------------------------------------- what the device builders are tried on
class Prims:
    """the scene stand-in of test_bvh_on_subdivided_mesh: triangles are one object, every sphere is an object of its own (as the parser packs them)"""
    def __init__(self, tris, spheres=None):
        tris = np.ascontiguousarray(tris, F32).reshape(-1, 3, 3)
        rows = [[0, tris.shape[0], 0]]
        if spheres is not None:
            spheres = np.ascontiguousarray(spheres, F32).reshape(-1, 4)
            rec = np.zeros((spheres.shape[0], 3, 3), F32)
            rec[:, 0] = spheres[:, :3]; rec[:, 1] = spheres[:, 3:4]
            rows += [[tris.shape[0] + k, 1, 1] for k in range(spheres.shape[0])]
            tris = np.concatenate([tris, rec])
        self.prims, self.n_prims = tris, tris.shape[0]
        self.obj_info, self.n_objects = np.int32(rows), len(rows)


SOUP_SIZES = (2, 3, 16, 17, 33, 63, 64, 65, 255, 256, 257, 1000)
CASES = tuple(f"soup-{n}" for n in SOUP_SIZES) + ("mixed", "planar", "coincident", "ribbon", "outlier", "bunnies1", "bunnies1-centred")
QUALITY_CASES = ("bunnies1", "bunnies1-centred", "mixed", "soup-1000")


def _soup(n, seed):
    """n random triangles, edge ~0.2, in [-3, 3]^3"""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-2.85, 2.85, size=(n, 1, 3))
    return (c + rs.uniform(-0.15, 0.15, size=(n, 3, 3))).astype(F32)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> Prims (or, for the bunnies, the packed scene).  Seeded: the same arrays in every process."""
    if name.startswith("soup-"):
        n = int(name[5:])
        return Prims(_soup(n, 1000 + n))
    if name == "mixed":                                           # k_prim_boxes' sphere branch: radii 1e-3 .. 0.5, ten concentric, ten identical
        rs = np.random.RandomState(7)
        sph = np.concatenate([rs.uniform(-2.5, 2.5, size=(200, 3)), np.exp(rs.uniform(np.log(1e-3), np.log(0.5), size=(200, 1)))], axis=1)
        sph[180:190, :3] = sph[180, :3]
        sph[190:200] = sph[190]
        return Prims(_soup(600, 8), sph)
    if name == "planar":                                          # a 32 x 32 grid of triangle pairs in the plane y = 0.5: no extent on one Morton axis
        g = np.linspace(-2.0, 2.0, 33, dtype=F32)
        xs, zs = np.meshgrid(g, g, indexing="ij")
        P = np.stack([xs, np.full_like(xs, 0.5), zs], axis=-1)
        a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
        return Prims(np.concatenate([np.stack([a, b, c], axis=-2).reshape(-1, 3, 3), np.stack([a, c, d], axis=-2).reshape(-1, 3, 3)]))
    if name == "coincident":                                      # every key and every union area ties
        tri = F32([[[-1.0, -0.5, 0.25], [0.4, -0.5, 0.25], [-1.0, 1.1, 0.25]]])
        return Prims(np.concatenate([np.repeat(tri, 300, axis=0), tri + F32([0.3, 0.2, 0.8])]))
    if name == "ribbon":                                          # 5 000 equal triangles in a row along x (the chain case described at k_ploc_nn)
        tri = F32([[-0.125, -0.25, 0.5], [0.125, -0.25, 0.5], [-0.125, 0.0, 0.75]])
        return Prims(tri[None] + F32([0.125, 0, 0]) * (np.arange(5000, dtype=F32) - 2500)[:, None, None])
    if name == "outlier":                                         # soup-1000 + one triangle at x = 1e4: almost all primitives in one Morton cell
        far = F32([[[1e4, 0.0, 0.0], [1e4 + 0.2, 0.0, 0.0], [1e4, 0.2, 0.1]]])
        return Prims(np.concatenate([case("soup-1000").prims, far]))
    if name in ("bunnies1", "bunnies1-centred"):                  # a real mesh (5 950 triangles); moved so that it straddles the origin
        from adapt_amd.scene_pack import pack_scene
        from adapt_amd.synth import three_bunnies
        fs = pack_scene(*three_bunnies(1))
        assert not fs.obj_info[:, 2].any()
        shift = F32([-2.8, -2.7, -2.8]) if name.endswith("centred") else F32([0, 0, 0])
        return Prims(np.asarray(fs.prims, F32).reshape(-1, 3, 3) + shift)
    raise KeyError(name)
