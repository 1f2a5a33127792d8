"""The scenes and ray batches of tests/sweep_cases.py reach the edges they are built for - shown with the oracle and numpy alone, so that
a green tests/test_gpu_sweep_limits.py means the limits of sweep_wg and sweep_tile (csrc/traverse.hpp) were actually run at."""
import numpy as np
import pytest

import sweep_cases as sc


def _info(fs):
    return np.int32(fs.obj_info).reshape(-1, 3)


def test_object_and_primitive_counts_are_the_stated_ones():
    _, t34 = sc.scene("tile_34")
    _, t35 = sc.scene("tile_35")
    i34, i35 = _info(t34), _info(t35)
    assert len(i34) == 34 and t34.n_prims <= 96 and len(i35) == 35 and t35.n_prims == t34.n_prims + 1 <= 96
    assert np.array_equal(i35[:34], i34) and tuple(i35[34, 1:]) == (1, 0)                    # tile_34 and one lone triangle
    assert np.array_equal(t35.prims.reshape(-1, 9)[:t34.n_prims], t34.prims.reshape(-1, 9))
    mesh_counts = i34[i34[:, 2] == 0, 1]
    for n in (5, 6, 7, 12): assert (mesh_counts == n).sum() == 1, (n, mesh_counts)
    assert set(mesh_counts) == {1, 2, 5, 6, 7, 12} and (i34[:, 2] != 0).sum() == 3
    order = [int(c) if k == 0 else "sphere" for _, c, k in i34]
    spheres = [k for k, x in enumerate(order) if x == "sphere"]
    assert all(0 < k < 33 and order[k - 1] != "sphere" and order[k + 1] != "sphere" for k in spheres)      # each between two meshes
    assert order[order.index(5) + 1] == 6                                                    # 5 next to 6: one object without a list, one with
    _, tv = sc.scene("tile_34", volumetric=True)
    assert np.array_equal(_info(tv), i34) and getattr(tv, "med_i", None) is not None                          # the volumetric variant: the same lists

    _, fl = sc.scene("lists_130")
    il = _info(fl)
    listed = sc.listed_objects(fl)
    assert len(listed) >= 130 and len(il) > 34
    past = np.arange(len(il)) > listed[sc.SWEEP_MAX_LISTS - 1]
    assert ((il[:, 2] != 0) & past).any() and ((il[:, 2] == 0) & (il[:, 1] < sc.SWEEP_LIST_MIN) & past).any()      # unlisted objects after the 128th list
    assert ((il[:, 2] != 0) & ~past).any() and ((il[6:, 2] == 0) & (il[6:, 1] < sc.SWEEP_LIST_MIN) & ~past[6:]).any()      # ... and before it
    assert {6, 7, 9, 12} <= set(il[listed, 1])

    _, fk = sc.scene("keys_16")
    ik = _info(fk)
    assert len(ik) <= 34 and 32768 < fk.n_prims < 65536
    assert sorted(ik[6:, 1]) == [7920, 7920, 7920, 31680]
    assert ik[-1, 0] >= 32768 and ik[-2, 0] < 32768 < ik[-2, 0] + ik[-2, 1]                  # the last bunny whole, the level-3 one in part
    lo, hi = fk.obj_aabb[6:, 0].min(axis=0), fk.obj_aabb[6:, 1].max(axis=0)
    assert (lo >= -0.01).all() and (hi <= sc.ROOM).all()                                     # the bunnies stand inside the room

    _, ft = sc.scene("ties")
    it = _info(ft)
    assert len(it) == 34 and (it[:, 1] == 2).all() and (it[:, 2] == 0).all()


def test_the_tile_fits_the_lds_at_34_objects_and_not_at_35():
    lds = lambda nt, n_obj: nt * 40 + n_obj * (nt * 8 + 4) + 16                              # traverse.hpp APT_TILE_LDS_BYTES
    assert lds(512, 34) == 159896 <= 160 * 1024 < lds(512, 35) == 163996
    assert lds(256, 34) <= 160 * 1024                                                        # k_vshadow's 256-thread tile
    assert sc.tile_lds_bytes(512, 34) == lds(512, 34)
    for name in ("tile_34", "keys_16", "ties"):
        assert lds(512, sc.scene(name)[1].n_objects) <= 160 * 1024, name
    for name in ("tile_35", "lists_130"):
        assert lds(512, sc.scene(name)[1].n_objects) > 160 * 1024, name


def test_batches_have_the_stated_lengths_and_degenerate_rays():
    b = sc.batches("tile_34")
    o, d, tmax = b["random"]
    assert len(o) == 4099 and o.dtype == d.dtype == tmax.dtype == np.float32
    assert (d[:64, 1] == 0).all() and (d[64:128, 0] == 0).all() and (d[64:128, 2] == 0).all() and (o[64:96, 0] == 0).all()
    assert np.abs(np.linalg.norm(np.float64(d), axis=1) - 1).max() < 1e-6
    assert [len(b[f"random[:{n}]"][0]) for n in sc.PREFIXES] == [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
    assert all(np.array_equal(b[f"random[:{n}]"][1], d[:n]) for n in sc.PREFIXES)
    assert len(b["away"][0]) % sc.TILE_NT == 0 and all(len(v[0]) % sc.TILE_NT == 0 for k, v in b.items() if k.startswith("aimed"))


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_aimed_rays_all_pass_their_object_s_box_and_away_rays_pass_no_listed_box(name):
    _, fs = sc.scene(name)
    listed = sc.listed_objects(fs)
    aimed = [k for k in sc.batches(name) if k.startswith("aimed(")]
    assert len(aimed) == (3 if name == "ties" else len(sc.AIMED_AT[name]))
    for k in aimed:
        obj = int(k[6:-1])
        o, d, _ = sc.batches(name)[k]
        assert sc.slab_pass(o, d, fs.obj_aabb[obj:obj + 1]).all(), k                         # every ray of every 256- and 512-ray block
        if name != "ties": assert obj in listed
    if name == "lists_130":                                                                  # the first list, the last list, the first object past it
        assert [int(k[6:-1]) for k in aimed] == [int(listed[0]), int(listed[127]), int(listed[128])]
        # nothing in front of the first listed object culls it: only the walls precede it in scene order, and they lie behind its box
        assert listed[0] == 6
    o, d, _ = sc.batches(name)["away"]
    if len(listed): assert not sc.slab_pass(o, d, fs.obj_aabb[listed]).any()


def test_lists_130_random_rays_end_past_the_128th_list():
    _, fs = sc.scene("lists_130")
    listed = sc.listed_objects(fs)
    obj = sc.oracle_hits("lists_130", "random")[0]
    share = float(np.isin(obj, listed[sc.SWEEP_MAX_LISTS:]).mean())
    print(f"lists_130: closest hit in a listed object past list 128 for {share:.4f} of the random rays")
    assert share >= 0.12                                                                     # measured 0.1491 of 4099
    assert np.isin(obj, listed[:sc.SWEEP_MAX_LISTS]).mean() >= 0.10                          # measured 0.1352: the listed ones are hit too
    unlisted_past = np.setdiff1d(np.arange(listed[sc.SWEEP_MAX_LISTS - 1] + 1, fs.n_objects), listed)
    assert np.isin(obj, unlisted_past).any()


def test_keys_16_random_rays_end_on_primitives_with_bit_15_set():
    prim = sc.oracle_hits("keys_16", "random")[1]
    n = int((prim >= 32768).sum())
    print(f"keys_16: {n} of 4099 random rays end on a primitive >= 32768")
    assert n >= 300                                                                          # measured 390
    assert ((prim >= 32768) & (prim % 2 == 1)).any() and ((prim >= 32768) & (prim % 2 == 0)).any()      # both halves of a pair record
    for batch in ("aimed(8)", "aimed(9)"):
        assert (sc.oracle_hits("keys_16", batch)[1] >= 32768).sum() >= 256, batch


def test_ties_random_rays_meet_the_tile_s_redo_condition():
    """condition (a) of sweep_tile's redo rule: two objects' own hits within 1e-5 t + 1e-6 at the minimum.  Also counted: the rays whose
    sequential answer (the oracle's loop over the objects in order, culling against the running minimum) differs from the order-free
    minimum over (t, primitive) - what the redo exists for.  Measured: 1068 tied rays, 0 order-sensitive ones (zero is an acceptable
    outcome: the device test then shows that the redo path returns the same answer, not that only it could)."""
    o, d, _ = sc.batches("ties")["random"]
    _, prim, t, _, _ = sc.oracle_hits("ties", "random")
    t_obj, p_obj = sc.per_object_hits("ties", o, d)
    t_min = t_obj.min(axis=1)
    hit = np.isfinite(t_min)
    eps = np.float32(1e-5) * t_min + np.float32(1e-6)
    tied = hit & ((t_obj <= (t_min + eps)[:, None]).sum(axis=1) >= 2)
    first = np.argmin(t_obj, axis=1)                                                         # the first of equal t: the lowest object, so the lowest primitive
    p_free = np.where(hit, p_obj[np.arange(len(o)), first], -1)
    t_free = np.where(hit, t_min, np.float32(1e7))
    sensitive = (p_free != prim) | (t_free != t)
    print(f"ties: {int(tied.sum())} tied rays, {int(sensitive.sum())} order-sensitive rays of {len(o)}")
    assert tied.sum() >= 1000
    assert sensitive.sum() <= tied.sum() and not (sensitive & ~tied).any()                   # order can matter only where candidates tie
    stacks = (prim[tied] - 12) // 8
    assert set(stacks) == set(range(7))                                                      # every stack: coincident, offset, tilted
