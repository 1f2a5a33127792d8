"""The adaptive-sampling retirement rule in numpy, shared by tests/test_adaptive_host.py (CPU) and tests/test_gpu_adaptive.py (device).
Not collected by pytest (no `test_` prefix); nothing here needs a device."""
import numpy as np


def rule_error(s1, s2, n):
    """DESIGN.md §4.6, one more time: per channel mean = S1/n, var = max(S2/n - mean^2, 0) * n/(n-1), se = sqrt(var/n);
    e_p = max over channels of se / (mean + 1e-3); +inf where any channel's ratio is not finite or n < 2."""
    s1 = np.asarray(s1, np.float64); s2 = np.asarray(s2, np.float64); n = np.asarray(n, np.int64)
    out = np.full(n.shape, np.inf)
    for idx in np.ndindex(n.shape):
        k = int(n[idx])
        if k < 2:
            continue
        ratios = []
        for c in range(3):
            with np.errstate(all="ignore"):
                mean = s1[idx][c] / np.float64(k)
                v = s2[idx][c] / np.float64(k) - mean * mean
                v = np.float64(0.0) if v < 0.0 else v
                var = v * (np.float64(k) / (np.float64(k) - 1.0))
                ratios.append(np.sqrt(var / np.float64(k)) / (mean + 1e-3))
        if all(np.isfinite(r) for r in ratios):
            out[idx] = max(ratios)
    return out
