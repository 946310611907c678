"""The arithmetic of BrightnessMultiplicativeDevice, ContrastAugmentationDevice and GammaDevice as training/data_augmentation/color.py
had it before the device kernels (per (sample, channel) loops of elementwise operations, after batchgenerators' augment_* functions),
restated in numpy with its draws from np.random in its order.  Every function evaluates in the dtype it is given: float64 is the
yardstick of tests/test_intensity_gpu.py, float32 shows what that arithmetic itself loses in single precision.  A helper module
of the tests, not a test file."""
import numpy as np


def range_pick(lo, hi):
    if np.random.random() < 0.5 and lo < 1:
        return np.random.uniform(lo, 1)
    return np.random.uniform(max(lo, 1), hi)


def brightness_one(x, m, dtype):
    return x.astype(dtype) * dtype(m)


def contrast_one(x, f, preserve_range, dtype):
    x = x.astype(dtype)
    mn = x.mean()
    lo, hi = x.min(), x.max()
    x = (x - mn) * dtype(f) + mn
    return np.clip(x, lo, hi) if preserve_range else x


def gamma_one(x, g, invert, retain_stats, epsilon, dtype):
    x = x.astype(dtype)
    if invert:
        x = -x
    if retain_stats:
        mn, sd = x.mean(), x.std()
    lo = x.min()
    rng = x.max() - lo
    x = np.power((x - lo) / (rng + dtype(epsilon)), dtype(g)) * rng + lo
    if retain_stats:
        x = x - x.mean()
        x = x / (x.std() + dtype(1e-8)) * sd + mn
    return -x if invert else x


def apply_params(data, params, one, dtype):
    """one(x, parameter, dtype) on every (sample, channel) of data [N, C, ...] whose entry of params [N, C] is not NaN."""
    out = data.astype(dtype)
    for b in range(data.shape[0]):
        for c in range(data.shape[1]):
            if not np.isnan(params[b, c]):
                out[b, c] = one(data[b, c], params[b, c], dtype)
    return out


def _loop(N, C, p, per_channel, draw, one, data, dtype):
    """The per-sample loop the three classes shared: `np.random.uniform() < p` per sample, then one draw per channel (per_channel)
    or one for the sample, whose C channels are then transformed as ONE array.  -> (result or None, drawn parameters [N, C], NaN
    where nothing was drawn)."""
    params = np.full((N, C), np.nan)
    out = None if data is None else data.astype(dtype)
    for b in range(N):
        if np.random.uniform() < p:
            if per_channel:
                for c in range(C):
                    params[b, c] = draw()
                    if out is not None:
                        out[b, c] = one(data[b, c], params[b, c], dtype)
            else:
                params[b, :] = draw()
                if out is not None:
                    out[b] = one(data[b], params[b, 0], dtype)
    return out, params


def brightness(N, C, data=None, dtype=np.float64, multiplier_range=(0.75, 1.25), per_channel=True, p_per_sample=0.15):
    r = multiplier_range
    return _loop(N, C, p_per_sample, per_channel, lambda: np.random.uniform(r[0], r[1]), brightness_one, data, dtype)


def contrast(N, C, data=None, dtype=np.float64, contrast_range=(0.75, 1.25), preserve_range=True, per_channel=True, p_per_sample=0.15):
    r = contrast_range
    return _loop(N, C, p_per_sample, per_channel, lambda: range_pick(r[0], r[1]),
                 lambda x, f, dt: contrast_one(x, f, preserve_range, dt), data, dtype)


def gamma(N, C, data=None, dtype=np.float64, gamma_range=(0.7, 1.5), invert_image=False, per_channel=True, retain_stats=True,
          p_per_sample=0.3, epsilon=1e-7):
    r = gamma_range
    return _loop(N, C, p_per_sample, per_channel, lambda: range_pick(r[0], r[1]),
                 lambda x, g, dt: gamma_one(x, g, invert_image, retain_stats, epsilon, dt), data, dtype)
