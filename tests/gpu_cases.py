"""Case bodies shared by the two GPU parity modules: tests/test_gpu_parity.py runs them on the EXACT build, tests/test_gpu_fast.py on the
PRODUCT build (whichever library `adapt_amd._lib.use()` has selected when the body runs), each with its own tolerances
(tests/parity_bounds.py holds the ones more than one module reads).  A body renders and collects, then holds what it collected to the
bounds with the criteria at the top of this file, which take arrays and counter dicts only (tests/test_gpu_cases_host.py checks them
without a device).  Not collected by pytest (no `test_` prefix): pytest does not rewrite the asserts here, so each carries its own message."""
import contextlib
import os

import numpy as np

from conftest import ROOT, SCENES, golden, image_metrics, record_metric, scene_from_golden
from parity_bounds import COUNTER_TOL
from adapt_amd.scene_pack import make_config

COUNTER_KEYS = ("n_shade", "n_shadow", "n_draws")      # vertices shaded, light samples taken, random numbers drawn


# ---------------------------------------------------------------- the criteria: arrays and counter dicts in, AssertionError out
def counters_within(st, ost, rel=COUNTER_TOL[0], floor=COUNTER_TOL[1], keys=COUNTER_KEYS, label=None):
    """path statistics `st` of the device against `ost` of the oracle (or of a fixture) on the same stream: each within max(rel * oracle,
    floor).  No systematic deviation: coplanar faces, NaN slabs and the like are reproduced.  The defaults are the product build's
    tolerance (tests/test_gpu_settings_matrix.py holds every settings case to it)."""
    for k in keys:
        assert abs(st[k] - ost[k]) <= max(rel * ost[k], floor), (label, k, st[k], ost[k])


def image_within(acc, ref, spp, within, rel, non_finite=None, explain=None, label=None, report=None):
    """The image criterion: accumulations `acc` (device) and `ref` (oracle, fixture) of `spp` samples agree on >= `within` of the pixels to
    1e-3 (1 + |x|) per channel and to relMSE <= `rel` (conftest.image_metrics).  non_finite: None compares the images as they are (a NaN
    fails the criterion); "identical" and "explained" leave out the pixels that are not finite in either image (upstream lets +inf through,
    vanilla_renderer.py:119) - "identical" requires the two maps of finite components to be equal, "explained" hands images whose maps
    differ to `explain(acc, ref)` -> (ok, findings).  `report(m, a, b, fin)` sees the metrics and the compared images before anything is
    held to a bound.  -> the metrics"""
    assert non_finite in (None, "identical", "explained"), non_finite
    same_map = np.array_equal(np.isfinite(acc), np.isfinite(ref))
    a, b, fin = acc, ref, None
    if non_finite:
        assert same_map or non_finite != "identical", (label, "finite components differ", int((np.isfinite(acc) != np.isfinite(ref)).sum()))
        fin = np.isfinite(acc).all(axis=2) & np.isfinite(ref).all(axis=2)
        a, b = np.where(fin[..., None], acc, 0), np.where(fin[..., None], ref, 0)
    a, b = a / spp, b / spp
    m = image_metrics(a, b)
    if report:
        report(m, a, b, fin)
    assert m["frac_within"] >= within and m["relMSE"] <= rel, (label, m)
    if non_finite == "explained" and not same_map:
        ok, findings = explain(acc, ref)
        assert ok, (label, findings)
    return m


OTHER_SEED_FILM = (48, 48, 64)        # width, height, spp of the other-seed cross-check


def _rel(a, b, finite_only=False):
    if finite_only:
        fin = np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)
        a, b = a[fin], b[fin]
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))


def other_seed_criterion_exact(label, hip, cpu):
    """SURVEY 8(d) as the exact build holds it: the device estimator is the same estimator, not merely the same stream -- against a CPU render
    with ANOTHER seed its relMSE stays within 1.5x of the relMSE between two CPU renders with different seeds.  `hip`: the device image with
    seed 0, `cpu`: the oracle's images with seeds 0, 1, 2 (float64, divided by the sample count)."""
    noise = _rel(cpu[1], cpu[2])
    assert noise > 0 and _rel(hip, cpu[1]) <= 1.5 * noise and _rel(hip, cpu[2]) <= 1.5 * noise, (label, _rel(hip, cpu[1]), _rel(hip, cpu[2]), noise)
    assert _rel(hip, cpu[0]) <= 1e-4 < noise, (label, _rel(hip, cpu[0]), noise)      # and on the SAME seed it is the same image, far below the noise floor


def other_seed_criterion(label, hip, cpu, frac):
    """SURVEY 8(d)'s statistical cross-check on images already rendered at OTHER_SEED_FILM: `hip` the device image with seed 0, `cpu` the
    oracle's images with seeds 0, 1, 2 (float64, divided by the sample count).  `frac`: the same-seed bound as a fraction of the seed-to-seed
    noise floor, None for 8(d)'s 1e-4 outright.  (tests/test_gpu_settings_matrix.py applies it to the settings cases that get a same-stream
    bound of their own.)"""
    rel = lambda a, b: _rel(a, b, finite_only=True)
    noise = rel(cpu[1], cpu[2])
    same = rel(hip, cpu[0])
    record_metric(f"other-seed cross-check {label}", {"noise_cpu1_cpu2": noise, "cpu0_vs_cpu1": rel(cpu[0], cpu[1]), "cpu0_vs_cpu2": rel(cpu[0], cpu[2]), "hip_vs_cpu1": rel(hip, cpu[1]), "hip_vs_cpu2": rel(hip, cpu[2]), "hip_vs_cpu0_same_seed": same})
    # 8(d)'s sentence takes ONE pair of CPU renders as "the noise".  relMSE is a mean of squares and these scenes have heavy tails (a small sphere
    # light, aggressive roulette): one firefly in one seed moves a pair's distance by a factor of two or more - measured on features_b,
    # d(cpu1, cpu2) = 0.28 but d(cpu0, cpu1) = 0.58, CPU against CPU; on features_a the other way round, 0.24 against 0.045.  So the noise floor is
    # taken per comparison from the CPU itself: HIP (seed 0) against CPU seed k may be at most 1.5x as far as CPU seed 0 is from CPU seed k -
    # the same statement with the firefly on both sides of the inequality - and, as 8(d) words it, within 1.5x of the largest CPU pair distance.
    d01, d02 = rel(cpu[0], cpu[1]), rel(cpu[0], cpu[2])
    assert noise > 0 and rel(hip, cpu[1]) <= 1.5 * d01 and rel(hip, cpu[2]) <= 1.5 * d02, (label, rel(hip, cpu[1]), d01, rel(hip, cpu[2]), d02)
    assert max(rel(hip, cpu[1]), rel(hip, cpu[2])) <= 1.5 * max(noise, d01, d02), (label, rel(hip, cpu[1]), rel(hip, cpu[2]), noise, d01, d02)
    assert same <= (1e-4 if frac is None else frac * noise) < noise, (label, same, noise)      # and on the SAME seed it is the same image, far below the noise floor


# ---------------------------------------------------------------- set-up the parity modules share
@contextlib.contextmanager
def renderer_factory(parsed):
    """factory make(tag, **kw) -> Renderer; every renderer a test makes is closed when that test ends (a renderer holds several GiB of
    queues per render lane).  Each module wraps it in its `renderer` fixture."""
    from adapt_amd.renderer import Renderer
    made = []

    def make(tag, **kw):
        r = Renderer(*parsed(tag), **kw)
        made.append(r)
        return r
    try:
        yield make
    finally:
        for r in made:
            r.close()


def run_bench(n, extra, tmp_path, tag, torchrun=True, rank_args=("--single-device", "--backend", "gloo"), env=None, timeout=600):
    """bench.py --config c1 for one timed step with N ranks in a child process -> (its last JSON line, the image it dumped).  N > 1: under
    torch.distributed.run as the driver starts it (`torchrun`), or left to launch its own ranks; `rank_args`: what N > 1 adds to the
    command (the default puts every rank on cuda:0 and gathers over gloo).  env: the child's environment (default: this one's)."""
    import json
    import socket
    import subprocess
    import sys
    img = str(tmp_path / f"{tag}.npy")
    common = ["bench.py", "--gpus", str(n), "--config", "c1", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-exclusive-pass"] + list(extra) + ["--dump-image", img]
    cmd = [sys.executable] + common
    if n > 1:
        common += list(rank_args)
        cmd = [sys.executable] + common
        if torchrun:
            sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port)] + common
    if env is None:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line), np.load(img)


def render_with_oracle(r, oracle, rc, spp, host_threads=False):
    """render and collect: `spp` samples on the renderer and, on the same Philox stream, in the oracle (`host_threads`: on every host thread
    the oracle may use) -> (accumulation, counters, the oracle's accumulation, the oracle's counters)"""
    from oracle import binding as ob
    r.render(n_spp=spp)
    acc, st = r.color.to_numpy(), r.stats()
    ref, _, ost = oracle.render(rc, spp, threads=ob.num_threads() if host_threads else 0)
    return acc, st, ref, ost


def bvhref_scene(tag):
    """tests/golden/bvhref_<tag>.npz -> (scene 4-tuple, packed scene, fixture): cbox carries its arrays; the bunny scenes are rebuilt by
    adapt_amd.synth and checked by hash"""
    import hashlib
    from adapt_amd.scene_pack import pack_scene
    g = golden(f"bvhref_{tag}.npz")
    if "prims" in g:
        tup, _ = scene_from_golden(tag, prefix="bvhref")
    else:
        from adapt_amd.synth import three_bunnies
        tup = three_bunnies({"bunnies1": 1, "bunnies3": 3}[tag])
    fs = pack_scene(*tup)
    assert hashlib.sha256(np.ascontiguousarray(fs.prims).tobytes()).hexdigest() == str(g["prims_sha256"]), "the fixture was recorded on other geometry"
    return tup, fs, g


# ---------------------------------------------------------------- the bodies; each returns r.info() for the caller to assert its build
def image_vs_oracle_same_stream(renderer, parsed, oracle_scene, tag, w, h, spp, ov, within, rel, counters, counters_floor=0,
                                host_threads=False, metric=None, same_energy=False, exact_structure=False):
    """A scene at a small film against the oracle on the same Philox stream: image, exact sample counts, path structure.  metric:
    record_metric's name for the image figures; same_energy: the two means within 1 %; exact_structure: what only the reference's
    arithmetic delivers - no more lit samples than the oracle's, and the normalised framebuffer is accumulation / spp."""
    r = renderer(tag, width=w, height=h, **ov)
    rc = make_config(parsed(tag)[3], width=w, height=h, **ov)
    acc, st, ref, ost = render_with_oracle(r, oracle_scene(tag), rc, spp, host_threads)
    image_within(acc, ref, spp, within, rel, label=tag, report=(lambda m, a, b, fin: record_metric(metric, m)) if metric else None)
    assert st["n_samples"] == ost["n_samples"] == w * h * spp, (tag, st["n_samples"], ost["n_samples"])
    counters_within(st, ost, counters, counters_floor, label=tag)
    if same_energy:
        mean_a, mean_b = float(np.nanmean(acc / spp)), float(np.nanmean(ref / spp))
        assert abs(mean_a - mean_b) <= 0.01 * mean_b, (tag, mean_a, mean_b)
    if exact_structure:
        assert st["n_lit"] <= ost["n_lit"] and st["n_shadow_traced"] <= st["n_shadow"], (tag, st["n_lit"], ost["n_lit"], st["n_shadow_traced"], st["n_shadow"])
        assert r.cnt[None] == spp and np.array_equal(r.pixels.to_numpy(), acc / np.float32(spp)), (tag, r.cnt[None])
    return r.info()


def image_vs_reference_run(renderer, tag, within, rel, draws, draws_floor=0, first_sample=False):
    """Directly against the fixture recorded from the reference's own kernel (same Philox stream).  first_sample: the first sample alone is
    compared too (the fixture's `first_sample`), to `within`."""
    g = golden(f"scene_{SCENES[tag][2]}.npz")
    w, h, spp = int(g["width"]), int(g["height"]), int(g["spp"])
    r = renderer(tag, width=w, height=h, max_bounce=int(g["max_bounce"]))
    if first_sample:
        r.render(n_spp=1)
        m1 = image_metrics(r.color.to_numpy(), g["first_sample"])
        assert m1["frac_within"] >= within, (tag, "first sample", m1)
    r.render(n_spp=spp - 1 if first_sample else spp)
    image_within(r.pixels.to_numpy(), g["pixels"], 1, within, rel, label=tag)
    counters_within(r.stats(), {"n_draws": int(g["draws"].sum())}, draws, draws_floor, keys=("n_draws",), label=tag)
    return r.info()


def other_seed_images(renderer, parsed, oracle_scene, tag):
    """render and collect for the other-seed criteria, at OTHER_SEED_FILM -> (device image with seed 0, the oracle's images with seeds
    0, 1, 2 - float64, divided by the sample count -, r.info())"""
    w, h, spp = OTHER_SEED_FILM
    cpu = {}
    for seed in (0, 1, 2):
        rc = make_config(parsed(tag)[3], width=w, height=h, seed=seed)
        cpu[seed] = oracle_scene(tag).render(rc, spp)[0].astype(np.float64) / spp
    r = renderer(tag, width=w, height=h, seed=0)
    r.render(n_spp=spp)
    return r.pixels.to_numpy().astype(np.float64), cpu, r.info()


def full_size_parity(renderer, parsed, oracle_scene, capsys, tag, spp, within, rel, counters, non_finite, print_l2=False):
    """BASELINE configs[1] and [2] at their FULL size - 512x512, 1024 spp, 8 / 16 bounces - against the oracle on the same Philox stream,
    every pixel, and the path statistics; the figures are printed (the run of record is profiles/r0N_full_size_parity.log).
    non_finite: image_within's option; print_l2: the per-pixel L2 distance is printed too."""
    r = renderer(tag)
    info = r.info()
    assert (r.w, r.h) == (512, 512) and r.max_bounce == (8 if tag == "cbox" else 16), (r.w, r.h, r.max_bounce)
    rc = make_config(parsed(tag)[3])
    acc, st, ref, ost = render_with_oracle(r, oracle_scene(tag), rc, spp)
    title = "full size" if info["arithmetic"] == "exact" else "full size, product build"

    def report(m, a, b, fin):
        l2 = np.sqrt(((a - b) ** 2).sum(axis=2))
        with capsys.disabled():
            print(f"\n[{title}] {tag}: 512x512x{spp} spp  relMSE {m['relMSE']:.3e}  max|diff| {m['max_abs']:.3e}  pixels within 1e-3(1+x) {100 * m['frac_within']:.4f} %  "
                  + (f"per-pixel L2 mean {l2.mean():.3e} max {l2.max():.3e}  " if print_l2 else "") + f"non-finite pixels {int((~fin).sum())}  "
                  f"n_shade {st['n_shade']} / {ost['n_shade']}  n_shadow {st['n_shadow']} / {ost['n_shadow']}  n_draws {st['n_draws']} / {ost['n_draws']}")
    image_within(acc, ref, spp, within, rel, non_finite, lambda a, b: oracle_scene(tag).explain_non_finite(rc, a, b, spp), tag, report)
    assert st["n_samples"] == ost["n_samples"] == 512 * 512 * spp, (tag, st["n_samples"], ost["n_samples"])
    counters_within(st, ost, counters, 0, label=tag)
    return info


def full_frame_every_pixel(renderer, parsed, oracle_scene, tag, spp, within, rel, counters, metric):
    """A BASELINE config at its full film size and bounce count and a part of its 1024 spp against the oracle on the same Philox stream,
    EVERY pixel of the 512 x 512 film, un-gated; pixels whose finiteness differs: zero-pdf knife-edges and nothing else."""
    r = renderer(tag)
    assert (r.w, r.h) == (512, 512), (r.w, r.h)
    rc = make_config(parsed(tag)[3])
    acc, st, ref, ost = render_with_oracle(r, oracle_scene(tag), rc, spp, host_threads=True)
    report = lambda m, a, b, fin: record_metric(metric, dict(m, n_shade=st["n_shade"], n_shade_oracle=ost["n_shade"], non_finite=int((~fin).sum())))
    image_within(acc, ref, spp, within, rel, "explained", lambda a, b: oracle_scene(tag).explain_non_finite(rc, a, b, spp), tag, report)
    counters_within(st, ost, counters, 0, label=tag)
    return r.info()


def full_frame_vs_oracle_statistics(renderer, tag, scene, counters, tiles, within, rel):
    """BASELINE configs[1] / [2] at their FULL film size against the oracle's render of the same samples (tests/golden/fullsize_*.npz,
    tests/golden/gen/gen_fullsize_stats.py): path statistics, the 8 x 8 grid of tile means (to `tiles` of their mean), the image at 1/8
    resolution."""
    g = golden(f"fullsize_{tag}.npz")
    w, h, spp = int(g["width"]), int(g["height"]), int(g["spp"])
    r = renderer(scene, width=w, height=h, max_bounce=int(g["max_bounce"]))
    r.render(n_spp=spp)
    st = r.stats()
    assert st["n_samples"] == int(g["n_samples"]) == w * h * spp, (tag, st["n_samples"], int(g["n_samples"]))
    counters_within(st, {k: int(g[k]) for k in COUNTER_KEYS}, counters, 0, label=tag)
    img = r.pixels.to_numpy().astype(np.float64)
    img[~np.isfinite(img).all(axis=2)] = 0.0
    tile_means = img.reshape(w // 64, 64, h // 64, 64, 3).mean(axis=(1, 3))
    small = img.reshape(w // 8, 8, h // 8, 8, 3).mean(axis=(1, 3))
    assert np.abs(tile_means - g["tiles"]).max() <= tiles * g["tiles"].mean(), (tag, float(np.abs(tile_means - g["tiles"]).max() / g["tiles"].mean()))
    image_within(small, g["small"].astype(np.float64), 1, within, rel, label=tag)
    return r.info()


def c3_crop_vs_oracle(parsed, oracle_scene, spp, within, rel, counters, host_threads=False):
    """C3 (csphere, 512 x 512, 16 bounces, S = 4 light samples per vertex) on a 128 x 96 window of the full frame against the oracle, same
    stream"""
    from adapt_amd.renderer import Renderer
    em, arr, objs, cfg = parsed("balls_mono")
    cfg = dict(cfg); cfg["film"] = {"width": 512, "height": 512, "crop_x": 250, "crop_y": 200, "crop_rx": 64, "crop_ry": 48}
    r = Renderer(em, arr, objs, cfg)
    try:
        rc = make_config(cfg)
        _, st, ref, ost = render_with_oracle(r, oracle_scene("balls_mono"), rc, spp, host_threads)
        win = (slice(rc.start_x, rc.end_x), slice(rc.start_y, rc.end_y))
        assert st["n_samples"] == ost["n_samples"] == spp * 128 * 96, (st["n_samples"], ost["n_samples"])
        image_within(r.pixels.to_numpy()[win], (ref / np.float32(spp))[win], 1, within, rel)
        counters_within(st, ost, counters, 0)
        return r.info()
    finally:
        r.close()


def fixture_then_oracle(r, g, oracle, rc, oracle_spp, label, within, rel, draws_tol, stat_tol):
    """renderer `r` (a) against the accumulation and draw counts the reference's own render left in fixture `g`, same Philox stream, then
    (b) against the oracle at `oracle_spp` samples, where the path structure has to agree too -> (counters, the oracle's counters) of (b)"""
    spp = int(g["spp"])
    r.render(n_spp=spp)
    image_within(r.color.to_numpy(), g["accum"], spp, within, rel, label=label)
    counters_within(r.stats(), {"n_draws": int(g["draws"].sum())}, draws_tol, 0, keys=("n_draws",), label=label)
    r.clear()
    acc, st, ref, ost = render_with_oracle(r, oracle, rc, oracle_spp)
    image_within(acc, ref, oracle_spp, within, rel, label=label)
    counters_within(st, ost, stat_tol, 0, label=label)
    return st, ost


def volumetric_scene_vs_reference_run_and_oracle(tag, within=0.99, rel=1e-3, draws_tol=2e-3, stat_tol=5e-4):
    """One of the reference's vpt scenes / this repo's media coverage scenes (tests/golden/vptscene_<tag>.npz): (a) against the image the
    reference's own VolumeRenderer.render produced on the same Philox stream, (b) against the oracle at more samples, where the path
    structure has to agree too: vertices shaded, light samples taken, random numbers drawn."""
    from adapt_amd.renderer import VolumeRenderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    tup, g = scene_from_golden(tag, "vptscene")
    w, h = int(g["width"]), int(g["height"])
    r = VolumeRenderer(*tup, width=w, height=h)
    try:
        assert r.info()["shade_variant"].startswith("volumetric"), r.info()["shade_variant"]
        rc = make_config(tup[3], width=w, height=h, volumetric=True)
        st, ost = fixture_then_oracle(r, g, ob.OracleScene(pack_scene(*tup), rc.cam_t), rc, 16, tag, within, rel, draws_tol, stat_tol)
        assert st["n_samples"] == ost["n_samples"] == w * h * 16, (tag, st["n_samples"], ost["n_samples"])
        # the walk only follows light samples that can contribute, the reference follows all of them
        assert 0 < st["n_track"] <= ost["n_track"] and st["n_lit"] <= ost["n_lit"] * (1 + stat_tol), (tag, st["n_track"], ost["n_track"], st["n_lit"], ost["n_lit"])
        return r.info()
    finally:
        r.close()


def grid_volume_vs_reference_run_and_oracle(name, within=0.985, rel=2e-3, draws_tol=3e-3, stat_tol=2e-3):
    """Grid volumes on the device (scenes/test/volgrid_*.xml): delta tracking in the free-path step and ratio tracking inside the light
    sampling draw from the path's own Philox stream in the reference's order, so image, vertices shaded, light samples and draw counts
    follow the oracle (and the reference-run fixture) like every other scene."""
    from adapt_amd.parsers.xml_parser import scene_parsing
    from adapt_amd.renderer import VolumeRenderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    g = golden(f"vptrun_{name}.npz")
    cwd = os.getcwd(); os.chdir(ROOT)
    try:
        tup = scene_parsing(os.path.join(ROOT, "scenes", "test"), name + ".xml")
        w, h = int(g["width"]), int(g["height"])
        r = VolumeRenderer(*tup, width=w, height=h)
        fs = pack_scene(*tup)
    finally:
        os.chdir(cwd)
    try:
        assert "grid volume" in r.info()["shade_variant"], r.info()["shade_variant"]
        rc = make_config(tup[3], width=w, height=h, volumetric=True)
        fixture_then_oracle(r, g, ob.OracleScene(fs, rc.cam_t), rc, 16, name, within, rel, draws_tol, stat_tol)
        return r.info()
    finally:
        r.close()


def _crop_vs_brute_force_oracle(tup, film, spp, name, within, rel, counters, reference_bvh):
    """A window of a large scene's full film, HIP (own BVH) vs the oracle's BRUTE-FORCE intersector on the same Philox stream: per pixel,
    exact sample counts, path statistics.  reference_bvh: the counters go into the metric, and the oracle renders the window once more
    through its restatement of the reference's BVH - the same picture up to that walk's rare lost hits."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    em, arr, objs, cfg = tup
    cfg = dict(cfg); cfg["film"] = film
    size = (2 * film["crop_rx"], 2 * film["crop_ry"])
    r = Renderer(em, arr, objs, cfg)
    try:
        info = r.info()
        assert info["traversal"] == "bvh", info["traversal"]
        rc = make_config(cfg)
        assert rc.do_crop and rc.use_bvh and (rc.end_x - rc.start_x, rc.end_y - rc.start_y) == size, (rc.do_crop, rc.use_bvh, size)
        win = (slice(rc.start_x, rc.end_x), slice(rc.start_y, rc.end_y))
        sc = ob.OracleScene(pack_scene(em, arr, objs, cfg), rc.cam_t, build_bvh=reference_bvh)
        rc.use_bvh = False
        acc, st, ref, ost = render_with_oracle(r, sc, rc, spp, host_threads=True)
        extra = dict(n_shade=st["n_shade"], n_shade_oracle=ost["n_shade"], n_draws=st["n_draws"], n_draws_oracle=ost["n_draws"]) if reference_bvh else {}
        report = lambda m, a, b, fin: record_metric(f"{name} {size[0]}x{size[1]}x{spp} {info['arithmetic']} build", dict(m, **extra))
        image_within(acc[win], ref[win], spp, within, rel, report=report)
        assert st["n_samples"] == ost["n_samples"] == spp * size[0] * size[1], (st["n_samples"], ost["n_samples"])
        counters_within(st, ost, counters, 0)
        if reference_bvh:
            rc.use_bvh = True
            mb = image_metrics(acc[win] / spp, sc.render(rc, spp, threads=ob.num_threads())[0][win] / spp)
            assert mb["frac_within"] >= 0.97, mb
        return info
    finally:
        r.close()


def c4_crop_vs_brute_force_oracle(within=0.9995, rel=1e-9, draws_tol=1e-4):      # (defaults: the exact build, measured 100 %, 4.8e-13, counts equal)
    """BASELINE configs[3] stand-in at full geometry (95 050 triangles, 800 x 800), the central 160 x 120 window x 8 spp (what bench.py's
    parity leg renders): the HIP tree returns the brute-force hit.  (The reference's own BVH, as restated in the oracle, drops ~2e-4 of
    the hits on this scene - its node boxes are unpadded - so it is compared statistically, not per pixel.)"""
    from adapt_amd.synth import three_bunnies
    film = {"width": 800, "height": 800, "crop_x": 400, "crop_y": 400, "crop_rx": 80, "crop_ry": 60}
    return _crop_vs_brute_force_oracle(three_bunnies(), film, 8, "c4 crop", within, rel, draws_tol, reference_bvh=True)


def c5_crop_vs_brute_force_oracle(cx, cy, within=0.9995, rel=1e-9, stat_tol=2e-3):      # (defaults: the exact build, measured 100 %, 1e-15)
    """BASELINE configs[4] stand-in at full geometry (285 134 triangles, 1280 x 720, 16 bounces), a 96 x 64 window x 8 spp"""
    from adapt_amd.synth import bunny_field
    film = {"width": 1280, "height": 720, "crop_x": cx, "crop_y": cy, "crop_rx": 48, "crop_ry": 32}
    return _crop_vs_brute_force_oracle(bunny_field(), film, 8, f"c5 crop ({cx}, {cy})", within, rel, stat_tol, reference_bvh=False)
