"""numpy model of the denoiser (include/adapt_mi.h apt_denoise_cfg): what the device's two stages are held to.  Not
collected by pytest (no `test_` prefix).

Images are (w, h, 3) indexed [x, y], as `pixels.to_numpy()`; the guides are the dict `Renderer.aov()` returns.  The firefly filter is
float32 operation for operation (its decisions are comparisons of float32 distances and its replacement value a float32 sum in a fixed
order); the a-trous filter runs in the dtype asked for, float64 by default."""
import numpy as np

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])           # B3 spline taps at offsets -2 .. 2
DEFAULTS = {"firefly_threshold": 0.0, "iterations": 3, "sigma_n": 128.0, "sigma_z": 0.1, "sigma_a": 0.1, "sigma_c": 1.0, "demodulate": True}


def sanitise(img):
    """non-finite components count as 0"""
    img = np.asarray(img, np.float32)
    return np.where(np.isfinite(img), img, np.float32(0))


def firefly(img, threshold, with_margin=False):
    """post_processing.py:15-32 on the zero-padded image: a pixel keeps its value if any of its 8 neighbours lies within Euclidean rgb
    distance < threshold of it; otherwise it becomes the float32 sum of the 8 neighbours (first index outermost) / 8.
    with_margin: also min over the neighbours of |distance - threshold| per pixel (how close the decision was)."""
    src = sanitise(img)
    w, h, _ = src.shape
    pad = np.zeros((w + 2, h + 2, 3), np.float32)
    pad[1:-1, 1:-1] = src
    thr = np.float32(threshold)
    keep = np.zeros((w, h), bool)
    total = np.zeros((w, h, 3), np.float32)
    margin = np.full((w, h), np.inf)
    for kx in range(3):
        for ky in range(3):
            if kx == 1 and ky == 1:
                continue
            q = pad[kx:kx + w, ky:ky + h]
            e = q - src
            dist = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], dtype=np.float32)
            keep |= dist < thr
            margin = np.minimum(margin, np.abs(dist.astype(np.float64) - float(thr)))
            total = total + q
    out = np.where(keep[..., None], src, total / np.float32(8))
    return (out, keep, margin) if with_margin else out


def guides(aov, dtype=np.float64):
    """(albedo, unit normal, depth, hit) in `dtype` from Renderer.aov()"""
    return (np.asarray(aov["albedo"], dtype), np.asarray(aov["normal"], dtype), np.asarray(aov["depth"], dtype), np.asarray(aov["hit_fraction"]) > 0)


def demodulate(colour, aov, dtype=np.float64):
    a, _, _, hit = guides(aov, dtype)
    return np.where(hit[..., None], np.asarray(colour, dtype) / np.maximum(a, 1e-3), np.asarray(colour, dtype))


def remodulate(colour, aov, dtype=np.float64):
    a, _, _, hit = guides(aov, dtype)
    return np.where(hit[..., None], np.asarray(colour, dtype) * np.maximum(a, 1e-3), np.asarray(colour, dtype))


def atrous_iteration(colour, aov, k, *, sigma_n=128.0, sigma_z=0.1, sigma_a=0.1, sigma_c=1.0, window=None, dtype=np.float64):
    """Iteration k (step 2^k) of the a-trous filter on `colour`: tap weight h(dx) h(dy) w_n w_z w_a w_c w_hit, taps outside the window
    (x0, x1, y0, y1; None: the film) skipped, the centre tap with h(0)^2, output = weighted sum / weight sum; pixels outside the window
    keep their value."""
    c = np.asarray(colour, dtype)
    a, n, z, hit = guides(aov, dtype)
    w, h, _ = c.shape
    x0, x1, y0, y1 = window if window is not None else (0, w, 0, h)
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    inside = (X >= x0) & (X < x1) & (Y >= y0) & (Y < y1)
    step = 1 << int(k)
    num = np.zeros_like(c)
    den = np.zeros((w, h), dtype)
    sc_k = sigma_c * 2.0 ** -int(k)
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            qx, qy = X + dx * step, Y + dy * step
            ok = (qx >= x0) & (qx < x1) & (qy >= y0) & (qy < y1)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            cq = c[qx, qy]
            wt = np.full((w, h), H5[dx + 2] * H5[dy + 2], dtype)
            if dx or dy:
                hq = hit[qx, qy]
                geo = np.maximum((n * n[qx, qy]).sum(-1), 0) ** sigma_n
                geo = geo * np.exp(-np.abs(z - z[qx, qy]) / (sigma_z * np.maximum(z, 1e-6)) - ((a - a[qx, qy]) ** 2).sum(-1) / sigma_a ** 2)
                wt = wt * np.where(hit, geo, 1.0) * (hq == hit)
                if sigma_c > 0:
                    wt = wt * np.exp(-((c - cq) ** 2).sum(-1) / sc_k ** 2)
            wt = np.where(ok, wt, 0)
            num += wt[..., None] * cq
            den += wt
    return np.where(inside[..., None], num / np.where(inside, den, 1)[..., None], c)


def denoise(colour, aov, *, window=None, dtype=np.float64, **cfg):
    """Both stages as apt_denoise chains them: non-finite -> 0, the firefly filter where firefly_threshold > 0, demodulation, K a-trous
    iterations, the albedo multiplied back."""
    unknown = set(cfg) - set(DEFAULTS)
    assert not unknown, unknown
    s = {**DEFAULTS, **cfg}
    c = sanitise(colour)
    if s["firefly_threshold"] > 0:
        c = firefly(c, s["firefly_threshold"])
    c = np.asarray(c, dtype)
    if s["demodulate"]:
        c = demodulate(c, aov, dtype)
    for k in range(int(s["iterations"])):
        c = atrous_iteration(c, aov, k, sigma_n=s["sigma_n"], sigma_z=s["sigma_z"], sigma_a=s["sigma_a"], sigma_c=s["sigma_c"], window=window, dtype=dtype)
    if s["demodulate"]:
        c = remodulate(c, aov, dtype)
    return c


def b3_spline_renormalised(img, k):
    """The plain separable B3-spline convolution at step 2^k with zero padding, divided by the same convolution of ones (border
    renormalisation): what an a-trous iteration reduces to when every edge-stopping weight is 1.  Written with 1-D passes, independently
    of atrous_iteration's 2-D tap loop."""
    img = np.asarray(img, np.float64)
    step = 1 << int(k)

    def along(arr, axis):
        out = np.zeros_like(arr)
        n = arr.shape[axis]
        for t, wgt in zip(range(-2, 3), H5):
            off = t * step
            lo, hi = max(0, -off), min(n, n - off)
            if lo >= hi:
                continue
            dst = [slice(None)] * arr.ndim; src = [slice(None)] * arr.ndim
            dst[axis], src[axis] = slice(lo, hi), slice(lo + off, hi + off)
            out[tuple(dst)] += wgt * arr[tuple(src)]
        return out

    num = along(along(img, 0), 1)
    den = along(along(np.ones(img.shape[:2]), 0), 1)
    return num / den[..., None]
