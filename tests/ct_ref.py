"""numpy restatements of the reference's CT case preparation, written from its definitions (TEST REFERENCE ONLY):
`DefaultPreprocessor.collect_foreground_intensities` (light_training/preprocessing/preprocessors/default_preprocessor.py:413-451),
`CTNormalization.run` (normalization/default_normalization_schemes.py:83-95), `run_case_npy` with it (:154-227) and `run_plan`
(:347-410) with `determine_fullres_target_spacing` (:304-333) and `compute_new_shape` (:335-345).  Also the synthetic inputs the CT
tests share."""
import math

import numpy as np

from tests import preprocess_ref as R

SEGMENT = 4096                                        # SEGM_FG_SEGMENT


# ---- the fingerprint of a case ----------------------------------------------------------------------------------------------------------
def foreground(segmentation, images):
    """:431-434: per channel `images[c][segmentation[0] > 0]`, C order of the logical volume"""
    mask = np.asarray(segmentation)[0] > 0
    return [np.asarray(images[c])[mask] for c in range(len(images))]


def collect_foreground_intensities(segmentation, images, seed=1234, num_samples=10000):
    """:413-451 as written there: ONE RandomState for all channels, `rs.choice(..., replace=True)`, numpy's statistics"""
    rs = np.random.RandomState(seed)
    samples, stats = [], []
    for fg in foreground(segmentation, images):
        n = len(fg)
        samples.append(rs.choice(fg, num_samples, replace=True) if n > 0 else [])
        with np.errstate(all="ignore"):               # numpy's float32 mean of the widest test channel overflows; it is not compared
            stats.append(_numpy_statistics(fg, n))
    return samples, stats


def _numpy_statistics(fg, n):
    return {
        "mean": np.mean(fg) if n > 0 else np.nan,
        "median": np.median(fg) if n > 0 else np.nan,
        "min": np.min(fg) if n > 0 else np.nan,
        "max": np.max(fg) if n > 0 else np.nan,
        "percentile_99_5": np.percentile(fg, 99.5) if n > 0 else np.nan,
        "percentile_00_5": np.percentile(fg, 0.5) if n > 0 else np.nan,
    }


def percentile_neighbours(sorted_fg, q):
    """the two order statistics np.percentile(..., q) interpolates between (method 'linear')"""
    n = len(sorted_fg)
    h = (n - 1) * (q / 100.0)
    lo = int(math.floor(h))
    return sorted_fg[lo], sorted_fg[min(lo + 1, n - 1)]


def percentile64(fg, q):
    """the contract's percentile: numpy's float64 interpolation on the float32 values, rounded once to float32"""
    return np.float32(np.percentile(np.asarray(fg).astype(np.float64), q))


def mean_bound(fg):
    """2^-24 |m| + 2^-40 mean|x|: the one rounding of the float64 mean m to float32, and the fp64 accumulation of n terms"""
    x = np.asarray(fg, dtype=np.float64)
    return 2.0 ** -24 * abs(float(x.mean())) + 2.0 ** -40 * float(np.abs(x).mean())


# ---- CT normalisation -----------------------------------------------------------------------------------------------------------------
def ct_normalize32(x, props):
    """CTNormalization.run (:83-95) in the fp32 form it was checked bit-equal to:
    (minimum(maximum(x, f32(lower)), f32(upper)) - f32(mean)) / f32(max(std, 1e-8))"""
    x = np.asarray(x, dtype=np.float32)
    lower, upper = np.float32(props["percentile_00_5"]), np.float32(props["percentile_99_5"])
    mean, std = np.float32(props["mean"]), np.float32(max(props["std"], 1e-8))
    return (np.minimum(np.maximum(x, lower), upper) - mean) / std


def ct_normalize_literal(x, props):
    """the reference's lines themselves (:88-94)"""
    image = np.asarray(x).astype(np.float32)
    image = np.clip(image, props["percentile_00_5"], props["percentile_99_5"])
    return (image - props["mean"]) / max(props["std"], 1e-8)


def run_case_ct(data, seg, spacing, props, out_spacing=(1, 1, 1), all_labels=(1, 2, 3)):
    """run_case_npy (:154-227) without resampling: crop to non-zero with the -1 rule, CT normalisation of the crop, class locations,
    the int8 / int16 choice.  -> (data fp32, seg, properties)"""
    d, s, bb, _ = R.crop_to_nonzero(np.asarray(data, dtype=np.float32), None if seg is None else np.asarray(seg, dtype=np.float32))
    out = np.stack([ct_normalize32(d[c], props[str(c)]) for c in range(d.shape[0])])
    locs = R.sample_locations(s, all_labels)
    s = s.astype(np.int16 if s.max() > 127 else np.int8)
    p = {"original_spacing_trans": [float(v) for v in list(spacing)[::-1]], "target_spacing_trans": list(out_spacing),
         "shape_before_cropping": list(data.shape[1:]), "bbox_used_for_cropping": bb,
         "shape_after_cropping_before_resample": list(d.shape[1:]), "shape_after_resample": list(d.shape[1:]), "class_locations": locs}
    return out, s, p


# ---- the plan of a dataset ------------------------------------------------------------------------------------------------------------
def determine_fullres_target_spacing(spacings, sizes):
    """:304-333 -> (target, whether the anisotropic branch was taken)"""
    target = np.percentile(np.vstack(spacings), 50, 0)
    target_size = np.percentile(np.vstack(sizes), 50, 0)
    worst = int(np.argmax(target))
    others = [i for i in range(len(target)) if i != worst]
    other_spacings = [target[i] for i in others]
    other_sizes = [target_size[i] for i in others]
    aniso = bool(target[worst] > 3 * max(other_spacings) and target_size[worst] * 3 < min(other_sizes))
    if aniso:
        t = np.percentile(np.vstack(spacings)[:, worst], 10)
        if t < max(other_spacings):
            t = max(max(other_spacings), t) + 1e-5
        target[worst] = t
    return target, aniso


def compute_new_shape(old_shape, old_spacing, new_spacing):
    """:335-345: both spacings reversed to the shape's order"""
    return np.array([int(round(i / j * k)) for i, j, k in zip(list(old_spacing)[::-1], list(new_spacing)[::-1], old_shape)])


def run_plan(spacings, sizes, samples_per_case):
    """:347-410 without `target medium patch size`; samples_per_case[case][channel] = the drawn samples or []"""
    channels = len(samples_per_case[0])
    pooled = [np.concatenate([r[i] for r in samples_per_case]) for i in range(channels)]
    stats = {}
    for i in range(channels):
        stats[i] = {"mean": float(np.mean(pooled[i])), "median": float(np.median(pooled[i])), "std": float(np.std(pooled[i])),
                    "min": float(np.min(pooled[i])), "max": float(np.max(pooled[i])),
                    "percentile_99_5": float(np.percentile(pooled[i], 99.5)), "percentile_00_5": float(np.percentile(pooled[i], 0.5))}
    target, aniso = determine_fullres_target_spacing(spacings, sizes)
    median_shape = np.median([compute_new_shape(j, i, target) for i, j in zip(spacings, sizes)], 0)
    tmp = 1 / np.array(target)
    patch = [round(i) for i in tmp * (256 ** 3 / np.prod(tmp)) ** (1 / 3)]
    return {"intensity_statistics_per_channel": stats, "fullres spacing": target.tolist(), "median_shape": median_shape.tolist(),
            "initial_patch_size": patch}, aniso


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def hu(shape, seed):
    """HU-like integers: heavy ties, both signs"""
    return np.round(300.0 * np.random.RandomState(seed).standard_normal(shape) - 200.0).astype(np.float32)


def blob(shape, centre=None, radii=None):
    """an ellipsoid; with the default centre and radii it straddles segment boundaries of a (19, 37, 53) volume"""
    centre = [n / 2.0 for n in shape] if centre is None else centre
    radii = [n / 3.0 for n in shape] if radii is None else radii
    g = np.ogrid[tuple(slice(0, n) for n in shape)]
    return sum(((a - c) / r) ** 2 for a, c, r in zip(g, centre, radii)) <= 1.0


def value_channels(shape, seed=3):
    """name -> one channel of the value patterns the selection must get right"""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    out = {"hu": hu(shape, seed), "mixed": (rng.standard_normal(shape) * np.exp(rng.uniform(-20, 20, shape))).astype(np.float32),
           "constant": np.full(shape, -37.5, dtype=np.float32)}
    # equal in the upper 22 bits of the key, different in the last digit only
    base = np.float32(1.5).view(np.uint32)
    out["last_digit"] = (base + rng.randint(0, 1024, n).astype(np.uint32)).view(np.float32).reshape(shape)
    # different in the top digit only: sign, exponent and three mantissa bits vary, the 20 bits below are one pattern
    top = rng.randint(0, 4096, n).astype(np.uint32)
    top = np.where((top >> 3) % 256 == 255, top ^ np.uint32(8), top)              # no infinities, no NaN
    out["top_digit"] = ((top << 20) | np.uint32(0x5a5a5)).view(np.float32).reshape(shape)
    z = rng.randint(-2, 3, shape).astype(np.float32)
    z[rng.random_sample(shape) < 0.3] = -0.0
    out["zeros"] = z
    return out


def ct_case(shape=(40, 44, 48), seed=0, labels=True):
    """a stand-in CT case: a body of HU-like values in air that is exactly 0, two labelled organs.  -> (data (1, D, H, W), seg)"""
    rng = np.random.RandomState(seed)
    body = blob(shape, radii=[n / 2.4 for n in shape])
    data = np.where(body, np.round(60.0 * rng.standard_normal(shape) + 40.0), 0.0).astype(np.float32)
    data[body & (data == 0)] = 1.0
    seg = np.zeros(shape, dtype=np.float32)
    if labels:
        c = [n / 2.0 for n in shape]
        organ = blob(shape, [c[0], c[1] - 4, c[2] - 5], [n / 6.0 for n in shape])
        lesion = blob(shape, [c[0] + 2, c[1] - 3, c[2] - 6], [n / 14.0 for n in shape])
        seg[organ], seg[lesion] = 1.0, 2.0
        data[organ] += 80.0
        data[lesion] -= 150.0
    return data[None], seg[None]
