"""The oracle under every sensor setting (tests/settings_cases.py) against the reference's own kernel run with the same overrides
(tests/golden/settings_matrix.npz, `gen_goldens.py --only settings`): accumulated image and every sample's draw count, bit for bit -
the standard tests/test_oracle_golden.py holds at the scene files' own settings.  The device tests of the matrix
(tests/test_gpu_settings_matrix.py) lean on the oracle; this module is what entitles them to."""
import numpy as np
import pytest

import settings_cases as SC
from conftest import golden
from adapt_amd.scene_pack import make_config, pack_scene
from oracle import binding as ob

G = golden("settings_matrix.npz")


def test_the_table_covers_what_it_claims():
    """every axis value on each of the three full-matrix scenes, the subset on the two others, the pairs; and the fixture holds exactly
    the table's cases with the settings the table gives them (no case is skipped, none is stale)"""
    assert set(SC.AXES) == set(SC.FLAG_AXES) | {f"shadow_{s}" for s in (0, 1, 2, 3, 5, 8)} | {"bounce_1", "bounce_2"}
    for scene in ("cbox", "balls_mono", "media_a"):
        have = {c.axis: c for c in SC.cases_of(scene)}
        for axis, ov in SC.AXES.items():
            assert axis in have, (scene, axis)
            st = SC.settings(have[axis])
            assert all(st[k] == v for k, v in ov.items()), (scene, axis, st)
    for scene in ("glass_box", "features_a"):
        assert {c.axis for c in SC.cases_of(scene)} == {"mis_off", "two_sided", "rr_off", "shadow_2", "shadow_5"}
    for scene in ("cbox", "balls_mono"):
        assert set(SC.PAIRS) <= {c.axis for c in SC.cases_of(scene)}
    assert SC.settings(SC.BY_NAME["cbox-mis_off"])["max_bounce"] == 8             # cbox: both sides get max_bounce explicitly
    assert sorted(G["names"].tolist()) == sorted(c.name for c in SC.CASES) and len(SC.CASES) == 66
    assert (int(G["width"]), int(G["height"]), int(G["spp"]), int(G["seed"])) == (SC.FIXTURE_W, SC.FIXTURE_H, SC.FIXTURE_SPP, SC.FIXTURE_SEED)
    for c in SC.CASES:
        st = SC.settings(c)
        assert SC.within_queue_limit(st["num_shadow_ray"], st["max_bounce"])
        for k in SC.SETTING_KEYS:                                                 # the reference's renderer was created with these settings
            assert float(G[f"{c.name}:{k}"]) == float(st[k]), (c.name, k)
    # a flipped setting changes the reference's own render: of the axis values every scene has, rr off and two and five light samples give
    # three different images, MIS off a fourth wherever a light has an area (the Cornell box's point light always weighs 1; and no scene
    # here shows a surface from behind, so two-sided BRDFs alone reproduce the scene's own image - in the reference as well)
    for scene in SC.SCENES:
        axes = ("rr_off", "shadow_2", "shadow_5") + (() if scene == "cbox" else ("mis_off",))
        assert len({G[f"{scene}-{a}:accum"].tobytes() for a in axes}) == len(axes), scene


_scenes = {}


def oracle_scene(scene):
    if scene not in _scenes:
        tup = SC.parse(scene)
        _scenes[scene] = ob.OracleScene(pack_scene(*tup), make_config(tup[3]).cam_t)
    return _scenes[scene]


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_oracle_reproduces_the_reference_run(name):
    case = SC.BY_NAME[name]
    w, h, spp, seed = SC.FIXTURE_W, SC.FIXTURE_H, SC.FIXTURE_SPP, SC.FIXTURE_SEED
    rc = make_config(SC.with_overrides(SC.parse(case.scene), case.overrides)[3], width=w, height=h, seed=seed, volumetric=case.volumetric)
    sc = oracle_scene(case.scene)
    acc, cnt, st = sc.render(rc, spp)
    ref, draws = G[f"{name}:accum"], G[f"{name}:draws"]
    assert cnt == spp and st["n_samples"] == w * h * spp
    assert np.array_equal(np.isnan(acc), np.isnan(ref))
    same = (acc.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(acc) & np.isnan(ref))
    assert same.all(), (name, int((~same.all(axis=-1)).sum()))
    got = np.zeros_like(draws)
    for s in range(spp):
        for i in range(w):
            for j in range(h):
                got[s, i, j] = sc.trace_sample(rc, i, j, s + 1)[2]
    assert np.array_equal(got, draws), (name, int((got != draws).sum()))
    assert st["n_draws"] == int(draws.sum())
    if rc.num_shadow_ray == 0:
        assert st["n_shadow"] == 0
