"""Inputs and independent truths for the grid-volume function tests (helper module: no tests in here).

  * volumes(): synthetic RGB grid volumes, packed exactly as a scene description carries them (vol_i[5], vol_f[33], grid [z][y][x][3]),
    with the majorant and its pdf by GridVolume_np.get_majorant's rule (max per channel, floored at 0.2 x the mean, x 1.05).
  * ray_rows() / density_rows(): the input rows of apt_volume_probe / orc_volume_probe, in named strata.
  * tau(): float64 quadrature of the field whose expectation the stochastic lookup is.  The lookup takes the voxel
    floor(index + (u - 0.5)) with u uniform: over u that is the trilinear interpolation of the voxel-centre values (voxel j's centre is
    at index j + 0.5), zero outside the grid.  No random number in it.
  * tracking_statistics(): the estimators' closed forms against that quadrature (see its docstring for every threshold).

Used by tests/test_volume_functions.py (CPU: oracle), tests/test_gpu_volume_functions.py (device, both builds) and
tests/golden/gen/gen_goldens.py --only volfunc (the reference's own GridVolume on the same rows).
"""
import math
import zlib

import numpy as np

F32 = np.float32
SEED_MFP, SEED_TR = 881, 882                # Philox seeds of the same-stream rows (mode 2 / mode 3)
STRATA = ("through", "inside", "clipped", "short", "miss", "zero1", "zero2", "graze")
THROUGHPUTS = F32([[1.0, 1.0, 1.0], [1.0, 0.05, 0.3], [0.7, 0.0, 0.4], [0.0, 0.0, 0.0]])      # white, strongly unequal, one channel zero, all zero
MAX_T = 100.0
VOLFUNC_PER, VOLFUNC_DENSITY = 8, 50          # rows per (volume, stratum) and lookups per volume in tests/golden/volume_functions.npz


def _rot(axis, deg):
    a = np.float64(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def pack(grid, albedo, rotation=None, scale=(1, 1, 1), offset=(0, 0, 0)):
    """(vol_i, vol_f, grid) as GridVolume_np.pack writes them: forward_t = rotation @ diag(scale), the box of the eight grid corners
    widened by 0.01, majorant = 1.05 * max(channel max, 0.2 * mean of the channel maxima), pdf = majorant / sum"""
    grid = np.ascontiguousarray(grid, F32)
    zres, yres, xres, _ = grid.shape
    fwd = (np.eye(3) if rotation is None else np.float64(rotation)) @ np.diag(np.float64(scale))
    x, y, z = xres, yres, zres
    corners = F32([[0, 0, 0], [x, 0, 0], [0, y, 0], [x, y, 0], [0, 0, z], [x, 0, z], [0, y, z], [x, y, z]])
    world = corners @ fwd.T + np.float64(offset)
    lo, hi = world.min(axis=0) - 0.01, world.max(axis=0) + 0.01
    maj = grid.max(axis=(0, 1, 2))
    maj = np.maximum(maj, np.mean(maj) * 0.2)
    maj = F32(maj * F32(1.05))
    vf = np.concatenate([F32(albedo), F32(np.linalg.inv(fwd)).reshape(-1), F32(offset), F32(lo), F32(hi), maj, F32(maj / maj.sum()),
                         F32([0, 0, 0]), F32([1, 0, 0])]).astype(F32)
    assert vf.shape == (33,)
    return np.int32([2, xres, yres, zres, 0]), vf, grid


def volumes():
    """name -> (vol_i, vol_f, grid).  Three different extents so an axis swap reads other memory; 1 x 1 x 1 and a flat 16 x 16 x 1;
    identity placements and one with rotation, anisotropic scale and offset; strong gradients with an empty region, a constant grid,
    and a colour ramp that leaves one channel identically zero in part of the box (make_colorful_volume does this upstream)."""
    rs = np.random.RandomState(zlib.crc32(b"volume_cases.volumes") & 0x7fffffff)
    out = {}
    # strong gradients, an empty region, rotated / anisotropically scaled / offset; albedos well away from 1
    z, y, x = np.meshgrid(np.arange(7), np.arange(9), np.arange(12), indexing="ij")
    blob = np.exp(-((x - 7.5) ** 2 / 6.0 + (y - 3.0) ** 2 / 4.0 + (z - 3.5) ** 2 / 3.0))
    g = (blob[..., None] * F32([9.0, 5.0, 2.5]) * rs.uniform(0.3, 1.0, size=(7, 9, 12, 3))).astype(F32)
    g[:, :, :3] = 0                                             # empty slab x < 3
    g[g < 0.05] = 0
    out["grad"] = pack(g, [0.9, 0.6, 0.3], _rot([1, 2, 0.5], 35.0), (0.30, 0.22, 0.41), (0.4, -1.1, 2.3))
    # constant grid, identity rotation: tau = sigma * length wherever the segment stays half a voxel inside the grid
    g = np.broadcast_to(F32([2.0, 1.2, 0.7]), (4, 5, 6, 3)).copy()
    out["const"] = pack(g, [0.8, 0.5, 0.95], None, (0.4, 0.4, 0.4), (-1.0, 0.5, 0.25))
    # colour ramp along z as upstream's mono2rgb: red is zero in the first slices, blue falls to zero in the last
    base = rs.uniform(0.5, 4.0, size=(10, 8, 6, 1)).astype(F32)
    half = 10 // 3
    ramp = np.ones((10, 3), F32)
    ramp[:half, 0] = 1 - np.linspace(1, 0, half, dtype=F32) ** 0.65
    ramp[half:, 2] = 1 - np.linspace(0, 1, 10 - half, dtype=F32) ** 0.6
    ramp[0, 0] = 0; ramp[-1, 2] = 0
    out["ramp"] = pack(base * ramp[:, None, None, :], [0.7, 0.85, 0.4], None, (0.35, 0.25, 0.2), (0.0, 0.0, 0.0))
    out["one"] = pack(np.full((1, 1, 1, 3), 1.0, F32) * F32([3.0, 0.5, 1.5]), [0.9, 0.9, 0.9], None, (2.0, 2.0, 2.0), (-1.0, -1.0, -1.0))
    g = (rs.uniform(0.0, 1.0, size=(1, 16, 16, 3)) ** 3 * 12.0).astype(F32)
    out["flat"] = pack(g, [0.99, 0.5, 0.1], _rot([0, 0, 1], 20.0), (0.2, 0.2, 0.6), (3.0, 0.0, -2.0))
    return out


# ------------------------------------------------------------------ input rows
def _unit(rs):
    d = rs.normal(size=3)
    return d / np.linalg.norm(d)


def _slab(lo, hi, o, d):
    """near / far of the box in float64 (finite directions only)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    return max(0.0, np.nanmax(np.minimum(t1, t2))), np.nanmin(np.maximum(t1, t2))


def _row(o, d, thp, max_t):
    return np.concatenate([F32(o), F32(d), F32(thp), F32([max_t])])


def ray_rows(vol, name, n_per):
    """-> {stratum: (n_per, 10) float32 rows o, d, thp, max_t} for one volume.  Every stratum draws from its own stream, row by row, so
    the first k rows do not depend on n_per.  The throughput cycles through THROUGHPUTS."""
    vf = vol[1]
    lo, hi = np.float64(vf[15:18]), np.float64(vf[18:21])
    c, h = (lo + hi) / 2, (hi - lo) / 2
    rad = float(np.linalg.norm(h))
    back = 2 * rad + 0.5
    out = {}
    for s in STRATA:
        rs = np.random.RandomState(zlib.crc32(f"{name}/{s}".encode()) & 0x7fffffff)
        rows = []
        for k in range(n_per):
            thp = THROUGHPUTS[k % 4]
            p = c + h * rs.uniform(-0.8, 0.8, size=3)            # a point inside the box
            d = _unit(rs)
            o, max_t = p - d * back, MAX_T
            if s == "inside":
                o = c + h * rs.uniform(-0.9, 0.9, size=3)
            elif s in ("clipped", "short"):
                near, far = _slab(lo, hi, np.float64(F32(o)), np.float64(F32(d)))
                max_t = near + rs.uniform(0.1, 0.9) * (far - near) if s == "clipped" else near * rs.uniform(0.2, 0.95)
            elif s == "miss":
                if k % 2:
                    d = -d                                       # the box lies behind the origin
                else:                                            # a line in a plane 1.2 box radii from the centre
                    n = _unit(rs)
                    d = np.cross(n, _unit(rs)); d /= np.linalg.norm(d)
                    o = c + n * rad * 1.2 - d * back
            elif s == "zero1":                                   # one direction component exactly zero: inv_dir = inf on that axis
                a = k % 3
                d[a] = 0.0; d /= np.linalg.norm(d)
                o = p - d * back
                o[a] = (lo[a], hi[a], hi[a] + 0.3, p[a])[(k // 3) % 4]      # on a face plane (0 * inf = NaN), outside the slab, inside it
            elif s == "zero2":                                   # axis-parallel
                a, b = k % 3, (k % 3 + 1 + (k // 3) % 2) % 3
                d = np.zeros(3); d[a] = 1.0 if (k // 6) % 2 else -1.0
                o = p - d * back
                o[b] = (lo[b], hi[b], lo[b] - 0.2, p[b], p[b])[(k // 12) % 5]
            elif s == "graze":                                   # cuts an edge of the box: the chord is 3e-5 .. 8e-5 long, near_t and far_t a few 1e-5 apart
                a = k % 3; b, e = (a + 1) % 3, (a + 2) % 3
                sb, se = rs.choice([-1.0, 1.0]), rs.choice([-1.0, 1.0])
                q = c.copy(); q[a] += h[a] * rs.uniform(-0.8, 0.8); q[b] += sb * h[b]; q[e] += se * h[e]      # on the edge
                L = rs.uniform(3e-5, 8e-5)
                inward = np.zeros(3); inward[b], inward[e] = -sb, -se
                d = np.zeros(3); d[b], d[e] = sb, -se; d /= np.linalg.norm(d)
                d[a] = rs.uniform(-0.2, 0.2); d /= np.linalg.norm(d)
                mid = q + inward / math.sqrt(2.0) * (L / 2)       # the chord's midpoint: L / 2 from the edge along the diagonal
                o = mid - d * rs.uniform(0.5, 2.0)
            rows.append(_row(o, d, thp, max_t))
        out[s] = F32(rows)
    return out


def density_rows(vol, name, n):
    """(n, 10) rows index xyz, u xyz, channel for the lookup: indices from three quarters of a voxel outside the grid on either side, some on
    integers and half-integers; u uniform, with the edge values 0, 0.5 and the largest float below 1"""
    vi = vol[0]
    res = np.float64(vi[1:4])
    rs = np.random.RandomState(zlib.crc32(f"{name}/density".encode()) & 0x7fffffff)
    rows = np.zeros((n, 10), F32)
    edge_u = F32([0.0, 0.5, np.nextafter(F32(1), F32(0)), 0.25])
    for k in range(n):
        idx = rs.uniform(-0.75, res + 0.75)
        u = rs.uniform(0, 1, size=3)
        if k % 5 == 1:
            idx = np.round(idx)
        if k % 5 == 2:
            idx = np.round(idx) + 0.5
        if k % 7 == 3:
            u[rs.randint(3)] = edge_u[rs.randint(4)]
        rows[k, 0:3], rows[k, 3:6], rows[k, 6] = idx, u, k % 3
    return rows


def same_stream_rows(n_per=80, n_density=120):
    """-> (groups, density): groups = list of (volume name, stratum, rows), density = list of (volume name, rows)"""
    vols = volumes()
    groups, dens = [], []
    for name, vol in vols.items():
        rr = ray_rows(vol, name, n_per)
        groups += [(name, s, rr[s]) for s in STRATA]
        dens.append((name, density_rows(vol, name, n_density)))
    return vols, groups, dens


# ------------------------------------------------------------------ the expectation of the lookup, and its line integral
def field(vol, idx, ch):
    """trilinear interpolation of the voxel-centre values of channel ch at voxel coordinates idx (..., 3), zero-padded: E_u[lookup]"""
    vi, _, grid = vol
    xres, yres, zres = int(vi[1]), int(vi[2]), int(vi[3])
    g = np.zeros((zres + 2, yres + 2, xres + 2))
    g[1:-1, 1:-1, 1:-1] = grid[..., ch]
    q = np.asarray(idx, np.float64) - 0.5                       # voxel j's centre sits at j + 0.5
    lim = np.float64([xres, yres, zres])
    q = np.clip(q, -1.0, lim)                                   # beyond one voxel outside everything is zero: clamp into the padding
    f = np.floor(q)
    w = q - f
    i = f.astype(np.int64) + 1                                  # index into the padded array
    i = np.minimum(i, np.int64([xres, yres, zres]))             # q == lim exactly: weight 0 on the far cell
    w = np.where(f >= lim, 1.0, w)
    ix, iy, iz = i[..., 0], i[..., 1], i[..., 2]
    wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
    acc = 0.0
    for dz, az in ((0, 1 - wz), (1, wz)):
        for dy, ay in ((0, 1 - wy), (1, wy)):
            for dx, ax in ((0, 1 - wx), (1, wx)):
                acc = acc + az * ay * ax * g[iz + dz, iy + dy, ix + dx]
    return acc


def to_local(vol, o, d):
    vf = np.float64(vol[1])
    inv_t = vf[3:12].reshape(3, 3)
    return inv_t @ (np.float64(o) - vf[12:15]), inv_t @ np.float64(d)


def tau_cumulative(vol, o, d, near, far, ch, n=1 << 15):
    """midpoint rule on n cells of [near, far]: (cell edges t (n + 1,), cumulative optical depth at them (n + 1,))"""
    ol, dl = to_local(vol, o, d)
    t = np.linspace(near, far, n + 1)
    mid = 0.5 * (t[1:] + t[:-1])
    s = field(vol, ol[None, :] + mid[:, None] * dl[None, :], ch)
    return t, np.concatenate([[0.0], np.cumsum(s) * ((far - near) / n)])


def tau(vol, o, d, near, far, ch, n=1 << 15):
    return float(tau_cumulative(vol, o, d, near, far, ch, n)[1][-1])


# ------------------------------------------------------------------ statistical rays
def stat_rays():
    """About 24 rays: three volumes x (through the body / origin inside / max_t ending inside), each with every tau_c(near, far) in
    [0.2, 3] where the estimators have power.  -> list of dicts name, kind, row (10,) float32.  Throughputs alternate between white and
    strongly unequal (every channel positive: a channel of zero throughput is never picked and has no estimator).  On the constant
    grid the `clipped` rays start and end half a voxel inside the grid, where tau = sigma * length in closed form."""
    vols = volumes()
    rays = []
    for name in ("grad", "const", "ramp"):
        vol = vols[name]
        vf = vol[1]
        lo, hi = np.float64(vf[15:18]), np.float64(vf[18:21])
        c, h = (lo + hi) / 2, (hi - lo) / 2
        back = 2 * float(np.linalg.norm(h)) + 0.5
        res = np.float64(vol[0][1:4])
        for kind in ("through", "inside", "clipped"):
            rs = np.random.RandomState(zlib.crc32(f"stat/{name}/{kind}".encode()) & 0x7fffffff)
            found = 0
            for _ in range(4000):
                if found == 3:
                    break
                d = _unit(rs)
                p = c + h * rs.uniform(-0.7, 0.7, size=3)
                o, max_t = p - d * back, MAX_T
                if name == "const" and kind == "clipped":            # both ends at least half a voxel inside the grid (identity rotation, scale 0.4)
                    core_lo, core_hi = np.float64(vf[12:15]) + 0.5 * 0.4, np.float64(vf[12:15]) + (res - 0.5) * 0.4
                    o = rs.uniform(core_lo, core_hi); e = rs.uniform(core_lo, core_hi)
                    d = (e - o) / np.linalg.norm(e - o); max_t = float(np.linalg.norm(e - o))
                elif kind == "inside":
                    o = c + h * rs.uniform(-0.6, 0.6, size=3)
                elif kind == "clipped":
                    near, far = _slab(lo, hi, o, d)
                    max_t = near + rs.uniform(0.4, 0.9) * (far - near)
                row = _row(o, d, THROUGHPUTS[len(rays) % 2], max_t)
                near, far = intersect64(vol, row)
                if not near < far:
                    continue
                taus = [tau(vol, row[0:3], row[3:6], near, far, ch, 1 << 12) for ch in range(3)]
                if min(taus) < 0.2 or max(taus) > 3.0:
                    continue
                rays.append({"name": name, "kind": kind, "row": row})
                found += 1
            assert found == 3, (name, kind, found)
    return vols, rays


def intersect64(vol, row):
    """near_t, far_t of vol_intersect in float64 (finite directions)"""
    vf = np.float64(vol[1])
    o, d = np.float64(row[0:3]), np.float64(row[3:6])
    near, far = _slab(vf[15:18], vf[18:21], o, d)
    return near + float(F32(1e-5)), min(float(row[9]), far) - float(F32(1e-5))


STAT_N, STAT_SEED = 1 << 16, 1000      # streams per ray; ray i uses seeds STAT_SEED + 2 i (ratio tracking) and + 2 i + 1 (delta tracking)
Z_MAX = 5.0                                         # every mean: within 5 standard errors
KS_MAX = math.sqrt(-math.log(0.5e-6) / 2.0)         # D sqrt(N) <= 2.69: the Dvoretzky-Kiefer-Wolfowitz bound at probability 1e-6


def tracking_statistics(probe, vol, ray, n, seed):
    """One ray, n independent streams (rows k = 0 .. n-1 of one probe call, keyed (k, seed)): every comparison of the estimators with
    the quadrature.  probe(mode, rows, seed) -> (n, 8).  Returns {label: (statistic, bound)}: the caller asserts statistic <= bound for
    every label and logs them.  With p_c = the normalised thp * pdf of channel c, e_c = exp(-tau_c(near, far)):

      tr_mean[c]      ratio tracking + roulette is unbiased, and the channel_vec(ch, Tr / p_ch) weighting cancels the pick:
                      E[out_c] = e_c; |mean - e_c| / (s / sqrt(n)) <= 5, s = the sample standard deviation of out_c over all streams
      mfp_channel[c]  frequency of channel c against p_c, 5 binomial standard errors
      mfp_free[c]     P(no collision | channel c) against e_c, 5 binomial standard errors
      mfp_ks[c]       sup |ECDF - F| sqrt(N_c) <= 2.69 over the collision distances of channel c, F(t) = 1 - exp(-tau_c(near, t)); streams
                      without a collision sit at +inf, so the ECDF is taken over all N_c streams and F is the (defective) CDF itself
      mfp_range       number of hit_t outside [near_t, far_t): 0
      mfp_beta[c]     E[beta_c] = albedo_c (1 - e_c) + e_c over all streams, 5 standard errors (sample standard deviation)
    """
    vf = np.float64(vol[1])
    row = ray["row"]
    rows = np.broadcast_to(row, (n, 10)).copy()
    near, far = [float(x) for x in probe(0, rows[:1], 0)[0, 1:3]]
    n64, f64 = intersect64(vol, row)
    assert abs(near - n64) <= 1e-5 * max(1.0, abs(n64)) and abs(far - f64) <= 1e-5 * max(1.0, abs(f64)), (near, n64, far, f64)
    pdfs = np.float64(row[6:9]) * vf[24:27]
    pdfs = pdfs / pdfs.sum()
    cum = [tau_cumulative(vol, row[0:3], row[3:6], near, far, ch) for ch in range(3)]
    half = [tau(vol, row[0:3], row[3:6], near, far, ch, 1 << 14) for ch in range(3)]
    e = np.array([math.exp(-cum[ch][1][-1]) for ch in range(3)])
    out = {}
    for ch in range(3):
        out[f"quadrature_halving[{ch}]"] = (abs(half[ch] - cum[ch][1][-1]), 1e-6)
    if ray["name"] == "const" and ray["kind"] == "clipped":           # closed form, no quadrature
        sigma = np.float64(vol[2][0, 0, 0])
        e = np.exp(-sigma * (far - near))
        for ch in range(3):
            out[f"closed_form_vs_quadrature[{ch}]"] = (abs(cum[ch][1][-1] - sigma[ch] * (far - near)), 1e-6)
    # ratio tracking
    tr = np.float64(probe(3, rows, seed)[:, 0:3])
    for ch in range(3):
        s = tr[:, ch].std(ddof=1)
        out[f"tr_mean[{ch}]"] = (abs(tr[:, ch].mean() - e[ch]) / (s / math.sqrt(n)), Z_MAX)
    # delta tracking
    m = probe(2, rows, seed + 1)
    hit_t, beta = np.float64(m[:, 0]), np.float64(m[:, 1:4])
    chan = np.argmax(beta != 0, axis=1)                                # beta = channel_vec(ch, Tr / pdf): Tr = 1 or albedo, never 0
    assert np.all((beta != 0).sum(axis=1) == 1)
    albedo = vf[0:3]
    bad = 0
    for ch in range(3):
        sel = chan == ch
        nc = int(sel.sum())
        out[f"mfp_channel[{ch}]"] = (abs(nc / n - pdfs[ch]) / math.sqrt(pdfs[ch] * (1 - pdfs[ch]) / n), Z_MAX)
        free = sel & (hit_t < 0)
        out[f"mfp_free[{ch}]"] = (abs(free.sum() / nc - e[ch]) / math.sqrt(e[ch] * (1 - e[ch]) / nc), Z_MAX)
        th = np.sort(hit_t[sel & (hit_t >= 0)])
        bad += int(((th < near) | (th >= far)).sum())
        F = 1.0 - np.exp(-np.interp(th, cum[ch][0], cum[ch][1]))
        k = np.arange(1, th.size + 1)
        D = max(np.max(np.abs(k / nc - F)), np.max(np.abs((k - 1) / nc - F)), abs(th.size / nc - (1 - e[ch])))
        out[f"mfp_ks[{ch}]"] = (D * math.sqrt(nc), KS_MAX)
        s = beta[:, ch].std(ddof=1)
        out[f"mfp_beta[{ch}]"] = (abs(beta[:, ch].mean() - (albedo[ch] * (1 - e[ch]) + e[ch])) / (s / math.sqrt(n)), Z_MAX)
    out["mfp_range"] = (float(bad), 0.0)
    return out


# ------------------------------------------------------------------ the float64 model on the same streams
def model_rows(vol, mode, rows, seed, stream, key0=0):
    """f64_models.volume_* over rows; row k reads the Philox stream (key0 + k, seed), sample 1, through stream(key, seed, sample, n) ->
    uint32 words (oracle.binding.rng_stream or adapt_amd.renderer.rng_stream).  -> (values (n, 8) float64 laid out as the probes lay
    them out, margin (n,): the smallest distance of a decision to its branch in units of its float32 error)"""
    import f64_models as M
    vi, vf, grid = vol
    out, margin = np.zeros((len(rows), 8)), np.zeros(len(rows))
    for k, row in enumerate(rows):
        if mode == 0:
            mg = M.Margin()
            hit, near, far, _, _ = M.volume_intersect(vf, row, mg)
            y = [float(hit), near, far]
        elif mode == 1:
            mg = M.Margin()
            y = [M.volume_density(vi, grid, row[0:3], row[3:6], int(row[6]), mg)]
        else:
            cache = {"w": stream(key0 + k, seed, 1, 64)}

            def words(i, cache=cache, key=key0 + k):
                while i >= len(cache["w"]):
                    cache["w"] = stream(key, seed, 1, 4 * len(cache["w"]))
                return cache["w"][i]
            y, mg = (M.volume_sample_mfp if mode == 2 else M.volume_transmittance)(vi, vf, grid, row, words)
        out[k, :len(y)] = y
        margin[k] = mg.m
    return out, margin


def compare_with_model(got, want, margin, mode, rel=2e-5):
    """rows of a float32 implementation against the model's: -> (safe (n,) bool: every decision further than f64_models.VOLUME_SAFE
    from its branch; ok (n,) bool: same draws, same channel and hit flag, values within rel, NaN for NaN)"""
    import f64_models as M
    got, want = np.float64(got), np.float64(want)
    width = {0: 3, 1: 1, 2: 5, 3: 4}[mode]
    with np.errstate(invalid="ignore"):
        close = (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= rel * np.abs(want)) | (got == want)
    ok = close[:, :width].all(axis=1)
    if mode >= 2:
        vec = slice(1, 4) if mode == 2 else slice(0, 3)
        ok &= ((got[:, vec] != 0) == (want[:, vec] != 0)).all(axis=1)
    return margin > M.VOLUME_SAFE, ok


def model_vs_oracle(n_per):
    """{(mode, stratum): (rows, share of rows whose draw count differs between the oracle and the float64 model, share of rows within
    VOLUME_SAFE of a branch, rows that are safe and still differ)}"""
    from oracle import binding as ob
    vols, groups, dens = same_stream_rows(n_per, 60)
    res = {}
    for mode, seed, draws in ((0, 0, None), (2, SEED_MFP, 4), (3, SEED_TR, 3)):
        acc = {s: [0, 0, 0, []] for s in STRATA}
        for name, vol in vols.items():
            rows = np.concatenate([r for n, s, r in groups if n == name])
            stratum = np.concatenate([[s] * len(r) for n, s, r in groups if n == name])
            o = ob.volume_probe(*vol, mode, rows, seed=seed)
            m, margin = model_rows(vol, mode, rows, seed, ob.rng_stream)
            safe, ok = compare_with_model(o, m, margin, mode)
            for s in STRATA:
                sel = stratum == s
                acc[s][0] += int(sel.sum())
                acc[s][1] += int((o[sel, draws] != m[sel, draws]).sum()) if draws is not None else int((o[sel, 0] != m[sel, 0]).sum())
                acc[s][2] += int((~safe[sel]).sum())
                acc[s][3] += [(name, int(k)) for k in np.nonzero(sel & safe & ~ok)[0]]
        for s in STRATA:
            n, a, b, c = acc[s]
            res[(mode, s)] = (n, a / n, b / n, c)
    return res


# ------------------------------------------------------------------ one analytic image through the renderer
ANALYTIC_W, ANALYTIC_H, ANALYTIC_SPP, ANALYTIC_BLOCK = 32, 24, 256, 8
ANALYTIC_LE = (3.0, 2.0, 1.0)


def analytic_scene():
    """One rectangular area emitter of constant radiance Le, facing the camera, seen through one purely absorbing grid volume
    (albedo 0), a world that does not scatter, nothing else in view, one bounce.  -> (scene tuple for Renderer / pack_scene, packed
    volume).

    What the loop computes (renderer/vpt.py:75-99 and 161-253; k_vevent and the event kernels on the device).  VolumeRenderer.sample_mfp
    takes the grid volume's result ONLY when it reports a collision (`if result[3] > 0: is_mi = 2; mfp = ...; beta = result[:3]`,
    vpt.py:93-98).  So a camera ray that collides gets throughput x channel_vec(ch, albedo / pdf) = 0, and the light sample taken at the
    collision is weighted by it; a ray that flies free keeps beta = (1, 1, 1) - the channel_vec(ch, 1 / pdf) the delta tracker returned
    is dropped - and collects Le with emission weight 1.  The emitter's own surface is black and max_bounce = 1 ends the path there.
    One sample is therefore X = Le * [free flight], the same Bernoulli variable for the three components, with
    P(free) = q = sum_k p_k exp(-tau_k), p = the majorant pdf (the camera throughput is white): the channel is picked first and the flight
    is free with the picked channel's transmittance.  E[pixel_c] = Le_c q averaged over the pixel's rays, E[X_c^2] = Le_c^2 q.
    (The spectrally resolved Le_c exp(-tau_c) would need the 1 / pdf weight on free flights; upstream does not apply it, and neither the
    oracle nor the device may.  The oracle's render of this scene is what settled it: per-channel means Le_c exp(-tau_c) miss it by
    up to 40 standard errors, Le_c q fits within 3.)  A ray that misses the volume's box draws nothing: X = Le."""
    import xml.etree.ElementTree as xet
    from adapt_amd.emitters import SOURCE_MAP
    from adapt_amd.synth import _Builder, _brdf
    from adapt_amd.volumes import GridVolume_np
    rs = np.random.RandomState(zlib.crc32(b"volume_cases.analytic") & 0x7fffffff)
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(8), indexing="ij")
    g = (rs.uniform(0.2, 1.0, size=(5, 6, 8, 3)) * F32([1.6, 1.0, 0.5]) * (0.3 + x[..., None] / 7.0)).astype(F32)
    g[:, :2, :, 1] = 0                                            # green empty in the lower third
    vol = pack(g, [0.0, 0.0, 0.0], _rot([0.2, 1, 0], 25.0), (0.45, 0.45, 0.45), (-1.7, -1.2, -0.9))

    class Packed(GridVolume_np):                                  # pack_scene asks a volume for pack() only
        def __init__(self, packed): self._packed = packed
        def pack(self): return self._packed

    b = _Builder()
    s, zq = 8.0, 3.0
    quad = F32([[[-s, -s, zq], [-s, s, zq], [s, s, zq]], [[-s, -s, zq], [s, s, zq], [s, -s, zq]]])      # normal -z: towards the camera
    b.mesh(quad, _brdf("lambertian", "#000000"), emitter=0)
    le = ", ".join(str(v) for v in ANALYTIC_LE)
    em = SOURCE_MAP["area"](xet.fromstring(f'<emitter type="area" id="quad"><rgb name="emission" value="{le}"/><rgb name="scaler" value="1.0"/></emitter>'))
    sensor = (f'<sensor><float name="fov" value="39.3077"/><integer name="max_bounce" value="1"/><integer name="num_shadow_ray" value="1"/>'
              f'<boolean name="use_rr" value="false"/><boolean name="anti_alias" value="true"/><boolean name="stratified_sampling" value="true"/>'
              f'<boolean name="use_mis" value="true"/><string name="accelerator" value="bvh"/><integer name="width" value="{ANALYTIC_W}"/>'
              f'<integer name="height" value="{ANALYTIC_H}"/></sensor>')
    emitters, arr, objs, cfg = b.finish([em], sensor)
    cfg["transform"] = (F32([0, 0, 1]), F32([0.0, 0.0, -6.0]), None)
    cfg["volume"] = [Packed(vol)]
    return (emitters, arr, objs, cfg), vol


def analytic_expectation(rc, vol, sub=4, steps=256):
    """-> (mean (w, h, 3), second moment (w, h, 3)) of one sample of the analytic scene (analytic_scene derives them), in float64: the camera model of pix2ray
    (direction cam_r @ ((half_w + vx - i) inv_focal, (j - half_h - vy) inv_focal, 1), normalised) at the centres of the sub x sub
    strata of each pixel, the optical depth by the midpoint rule on `steps` cells (a fiftieth of a voxel)."""
    w, h = rc.width, rc.height
    vf = np.float64(vol[1])
    off = (np.arange(sub) + 0.5) / sub
    i, j, a, bq = np.meshgrid(np.arange(w), np.arange(h), off, off, indexing="ij")
    cam = np.stack([(rc.half_w + a - i) * rc.inv_focal, (j - rc.half_h - bq) * rc.inv_focal, np.ones_like(a)], -1)
    d = cam @ np.float64(rc.cam_r).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.float64(rc.cam_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (vf[15:18] - o) / d, (vf[18:21] - o) / d
    near = np.maximum(0.0, np.minimum(t1, t2).max(-1)) + 1e-5
    far = np.maximum(t1, t2).min(-1) - 1e-5                       # the emitter lies behind the box
    hit = (near < far) & (far > 0)
    inv_t = vf[3:12].reshape(3, 3)
    ol, dl = inv_t @ (o - vf[12:15]), d @ inv_t.T
    frac = (np.arange(steps) + 0.5) / steps
    t = near[..., None] + (far - near)[..., None] * frac
    idx = ol + dl[..., None, :] * t[..., None]
    q = np.zeros(d.shape[:-1])
    for ch in range(3):
        tau_c = np.where(hit, field(vol, idx, ch).sum(-1) * (far - near) / steps, 0.0)
        q += vf[24 + ch] * np.exp(-tau_c)
    q = np.where(hit, q, 1.0)[..., None]
    le = np.float64(ANALYTIC_LE)
    return (le * q).mean(axis=(2, 3)), (le * le * q).mean(axis=(2, 3))


def analytic_z_scores(image, rc, vol, spp):
    """-> (block z-scores (w / B, h / B, 3) of a rendered mean image against analytic_expectation: (block mean - expected) / standard
    error, the error from the analytic second moment (stratified sampling can only lower it), 0 for a block without variance; the
    expected block means; the differences)"""
    B = ANALYTIC_BLOCK
    mean, second = analytic_expectation(rc, vol)
    blk = lambda a: a.reshape(rc.width // B, B, rc.height // B, B, 3).mean(axis=(1, 3))
    m, s2 = blk(mean), blk(second)
    var = s2 - blk(mean * mean)                                   # per-sample variance averaged over the block (each pixel has its own mean)
    se = np.sqrt(np.maximum(var, 0.0) / (B * B * spp))
    diff = blk(np.float64(image)) - m
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(se > 1e-12, diff / se, 0.0), m, diff


# ------------------------------------------------------------------ rows that sit exactly on a branch
def far_boundary_rows(probe, n=96):
    """Delta tracking accepts a collision only at t < far_t; t == far_t is not one.  No random ray lands there, so the rows are built from
    the implementation's own first step: on the constant grid (density / majorant = 1 / 1.05) the first tentative collision t1 is accepted
    on 19 rows of 20 and returned as hit_t (6 draws: channel, step, three lookup offsets, the collision test).  Each such row is run
    again, same stream, with max_t chosen among the floats around t1 + 1e-5 such that far_t = fl(max_t - 1e-5f) is exactly t1, and once
    more with the next float that puts far_t one ulp above t1.
    probe(mode, rows, seed) -> (n, 8).  -> (rows at the boundary, their outputs, rows one ulp inside, their outputs, t1)"""
    vol = volumes()["const"]
    vf = vol[1]
    rs = np.random.RandomState(zlib.crc32(b"volume_cases.far_boundary") & 0x7fffffff)
    lo, hi = np.float64(vf[12:15]) + 0.6, np.float64(vf[12:15]) + np.float64(vol[0][1:4]) * 0.4 - 0.6
    rows = F32([_row(rs.uniform(lo, hi), _unit(rs), THROUGHPUTS[k % 2], MAX_T) for k in range(n)])
    first = probe(2, rows, SEED_MFP)
    box_far = probe(0, rows, 0)[:, 2]
    eps = F32(1e-5)
    at, inside, keep = rows.copy(), rows.copy(), np.zeros(n, bool)
    for k in range(n):
        t1 = F32(first[k, 0])
        if not (first[k, 4] == 6 and t1 > 0 and t1 + 4 * eps < box_far[k]):
            continue
        c = F32(t1 + eps)
        cands = [c]
        for _ in range(8):
            cands = [np.nextafter(cands[0], F32(0))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
        on = [x for x in cands if F32(x - eps) == t1]
        above = [x for x in cands if F32(x - eps) > t1]
        if on and above:
            at[k, 9], inside[k, 9], keep[k] = on[0], above[0], True
    # keys are row indices: the kept rows stay where they are, the others keep MAX_T and are masked out
    out_at, out_in = probe(2, at, SEED_MFP), probe(2, inside, SEED_MFP)
    return keep, first, out_at, out_in


def check_far_boundary(probe):
    """a tentative collision exactly at far_t is not a collision (2 draws: channel and the step); one ulp below far_t it is the collision
    of the unclipped row.  -> rows checked"""
    keep, first, at, inside = far_boundary_rows(probe)
    assert keep.sum() >= 48, keep.sum()
    assert np.all(at[keep, 0] == -1) and np.all(at[keep, 4] == 2), (at[keep][:4], first[keep][:4])
    assert np.array_equal(inside[keep, :5], first[keep, :5])
    return int(keep.sum())


# Philox streams (row 0, seed, sample 1) whose SIXTH draw is exactly 1 / 16 (word >> 8 == 2^20): found by searching the seeds 0 .. 2^27 with
# a vectorised Philox4x32-10; tests/test_volume_functions.py re-derives the property through the oracle's generator.
ROULETTE_SEEDS = (8716829, 42993346, 43342851, 121163913)


def roulette_boundary():
    """Ratio tracking's roulette ends the walk when xi >= Tr; xi == Tr happens once in 2^24 roulettes, so it is constructed: a constant grid
    of density 15 with the majorant set to 16 (every value exact in float32: 1 / 16, 15 / 16, Tr = 1 - 15 / 16 = 1 / 16 < 0.1 after the
    first step) and streams whose sixth draw (channel, step, three lookup offsets, then the roulette) is 1 / 16.  -> (volume at the
    boundary, the same with the density one ulp lower (Tr one ulp above 1 / 16: the walk survives), the row)"""
    g = np.full((4, 5, 6, 3), 15.0, F32)
    at = pack(g, [0.5, 0.5, 0.5], None, (0.4, 0.4, 0.4), (0.0, 0.0, 0.0))
    below = pack(np.full((4, 5, 6, 3), np.nextafter(F32(15), F32(0)), F32), [0.5, 0.5, 0.5], None, (0.4, 0.4, 0.4), (0.0, 0.0, 0.0))
    for vol in (at, below):
        vol[1][21:24] = 16.0
        vol[1][24:27] = F32(1.0 / 3.0)
    d = np.float64([0.48, 0.6, 0.64])
    row = _row(np.float64([1.2, 1.0, 0.8]), d / np.linalg.norm(d), [1, 1, 1], MAX_T)
    return at, below, row


def check_roulette_boundary(probe):
    """probe(vol, mode, rows, seed) -> (n, 8)"""
    at, below, row = roulette_boundary()
    for seed in ROULETTE_SEEDS:
        a, b = probe(at, 3, row[None, :], seed)[0], probe(below, 3, row[None, :], seed)[0]
        assert tuple(a[:4]) == (0.0, 0.0, 0.0, 6.0), (seed, a)              # xi == Tr: killed at the sixth draw
        assert b[3] > 6, (seed, b)                                          # Tr one ulp larger: the same draw survives and the walk goes on
