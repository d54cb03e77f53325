"""Float64 numpy restatements of the five plane ops of csrc/intensity.hip, written the way segmamba_amd/augment.py writes them
(`SplineAugmenter.__call__` for noise, brightness and contrast, `SplineAugmenter._gamma` for the gammas).  A plane is any array; all
statistics are taken over all of its voxels.  Host parameters are fp32, as the kernels take them.  The one rounding the formulas name
themselves - u = fl32(v * m), the brightness that is folded into contrast - is taken in fp32 here too."""
import numpy as np


def noise_ref(v, n, s):
    """x += randn * s"""
    return v.astype(np.float64) + np.float64(np.float32(s)) * n.astype(np.float64)


def scale_ref(v, m):
    """x *= m"""
    return v.astype(np.float64) * np.float64(np.float32(m))


def contrast_ref(v, m, f):
    """u = fl32(v m); minimum(maximum((u - mean) f + mean, lo), hi)"""
    u = (v.astype(np.float32) * np.float32(m)).astype(np.float64)
    mn, lo, hi = u.mean(), u.min(), u.max()
    return np.minimum(np.maximum((u - mn) * np.float64(np.float32(f)) + mn, lo), hi)


def gamma_ref(v, g, invert):
    """`_gamma` with the population standard deviation (numpy.std, what the published transform uses)"""
    t = -v.astype(np.float64) if invert else v.astype(np.float64)
    mn, sd = t.mean(), t.std()
    lo = t.min()
    rng = t.max() - lo
    w = np.power(np.maximum((t - lo) / (rng + 1e-7), 0.0), np.float64(np.float32(g))) * rng + lo
    w = w - w.mean()
    w = w / (w.std() + 1e-8) * sd + mn
    return -w if invert else w


def stats_ref(x):
    """count, mean, population sd, min, max of a plane, in float64 on the fp32 data"""
    x = x.astype(np.float64)
    return np.array([x.size, x.mean(), x.std(), x.min(), x.max()])
