"""Intensity augmentation on the device kernels (csrc/intensity.hip, training/data_augmentation/color.py): `mt_channel_stats` against
numpy in float64, the three functional forms and the three classes against the float64 evaluation of the loops they replaced
(tests/intensity_restatement.py), untouched inactive channels, no device-to-host read, no CPU fallback.

Bound of the value tests, computed per case: max|device - f64| <= 4 * max(max|f32 restatement - f64|, ulp32(max|x|)) — four times
what the same arithmetic loses in numpy's own float32, for the few-ulp differences between the device's powf / division and
numpy's over a chain of at most eight roundings.  Every case prints its measured ratio (1.0 = numpy's own float32 deviation)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_restatement as IR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 11),        # smaller than one workgroup's share, with a tail
          (3, 33, 65),       # odd V: channels only dword-aligned, several workgroups
          (17, 63, 97)]      # odd V, many workgroups per channel
N, CN = 2, 3
INACTIVE = (0, 1)
_cache = {}


def _data(shape):
    """Seeded normal channels of different location and scale, the mean-100 / sd-1 channel and one constant channel (read only)."""
    if shape not in _cache:
        rs = np.random.RandomState(sum(shape))
        d = rs.randn(N, CN, *shape)
        d[0, 0] = d[0, 0] * 2 + 0.5
        d[0, 2] = d[0, 2] + 100.
        d[1, 0] = d[1, 0] * 0.1 - 3
        d[1, 2] = 3.
        d = d.astype(np.float32)
        d.setflags(write=False)
        _cache[shape] = d
    return _cache[shape]


def _active():
    a = np.ones((N, CN), dtype=bool)
    a[INACTIVE] = False
    return a


def _ratio(got, r32, r64, d, mask=None):
    """max|got - f64| over max(max|f32 - f64|, ulp32(max|x|)) on the channels of mask."""
    m = np.ones((N, CN), dtype=bool) if mask is None else mask
    base = max(float(np.abs(r32[m].astype(np.float64) - r64[m]).max()), float(np.spacing(np.float32(np.abs(d[m]).max()))))
    return float(np.abs(got[m].astype(np.float64) - r64[m]).max()) / base


@pytest.mark.parametrize('shape', SHAPES)
def test_channel_stats_against_float64(dev, shape):
    from multitalent_amd import _lib, ops
    d = _data(shape)
    x = torch.from_numpy(d.copy()).to(dev)
    act = _active()
    st = ops.channel_stats(x, act, torch.full((N * CN, 4), float('nan'), dtype=torch.float64, device=dev))
    again = ops.channel_stats(x, act, torch.full((N * CN, 4), float('nan'), dtype=torch.float64, device=dev))
    assert torch.equal(st.view(torch.int64), again.view(torch.int64))                  # bit-identical, NaN rows included
    assert torch.equal(x.cpu(), torch.from_numpy(d.copy()))
    got = st.cpu().numpy().reshape(N, CN, 4)
    assert np.isnan(got[INACTIVE]).all() and not np.isnan(got[act]).any()

    def check(row, v, tag):
        v = v.astype(np.float64).reshape(-1)
        mean, sd = v.mean(), v.std()
        print('stats %s %s: mean err %.3g (bound %.3g), sd err %.3g (bound %.3g)'
              % (shape, tag, abs(row[2] - mean), 1e-10 * np.abs(v).max(), abs(row[3] - sd), 1e-8 * sd))
        assert row[0] == v.min() and row[1] == v.max()
        assert abs(row[2] - mean) <= 1e-10 * np.abs(v).max()
        assert abs(row[3] - sd) <= 1e-8 * sd
    for b in range(N):
        for c in range(CN):
            if act[b, c]:
                check(got[b, c], d[b, c], (b, c))
    whole = ops.channel_stats(x.view(N, -1)).cpu().numpy()                            # a sample as one channel of C * V elements
    for b in range(N):
        check(whole[b], d[b], (b, 'all'))
    lib = _lib.load()
    need = lib.mt_channel_stats_workspace(N * CN, x[0, 0].numel())
    assert need >= N * CN * 32
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.mt_channel_stats(x.data_ptr(), N * CN, x[0, 0].numel(), None, st.data_ptr(), ws.data_ptr(), need - 1,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b'workspace' in lib.mt_last_error()                            # MT_EINVAL before any launch
    assert torch.equal(st.view(torch.int64), again.view(torch.int64))


def _functional_case(dev, d, fn, one, value, tag):
    """fn(x, params) in place with `value` for every channel but INACTIVE, which carries a NaN: the NaN stays where it is, the
    channel is bit-identical, nothing else becomes NaN, and the active channels meet the bound."""
    params = np.full((N, CN), float(value))
    params[INACTIVE] = np.nan
    src = d.copy()
    src[INACTIVE][1, 2, 3] = np.nan
    x = torch.from_numpy(src.copy()).to(dev)
    assert fn(x, params) is x
    got = x.cpu().numpy()
    assert got[INACTIVE].tobytes() == src[INACTIVE].tobytes()
    assert int(np.isnan(got).sum()) == 1
    act = _active()
    r64, r32 = IR.apply_params(src, params, one, np.float64), IR.apply_params(src, params, one, np.float32)
    assert np.isfinite(r64[act]).all() and np.isfinite(got[act]).all()
    ratio = _ratio(got, r32, r64, src, act)
    print('functional %s %s: ratio %.3f' % (d.shape[2:], tag, ratio))
    return ratio


@pytest.mark.parametrize('shape', SHAPES)
def test_functional_forms_against_the_float64_restatement(dev, shape):
    from multitalent_amd.training.data_augmentation import color
    d = _data(shape)
    worst = {}
    for m in (0.75, 1.25):
        worst['brightness %g' % m] = _functional_case(dev, d, color.augment_brightness_device, IR.brightness_one, m, 'brightness %g' % m)
    for preserve in (True, False):
        for f in (0.75, 1.25):
            tag = 'contrast f=%g preserve_range=%s' % (f, preserve)
            worst[tag] = _functional_case(dev, d, lambda x, p: color.augment_contrast_device(x, p, preserve_range=preserve),
                                          lambda v, q, dt: IR.contrast_one(v, q, preserve, dt), f, tag)
    for g in (0.7, 1.5):
        for invert in (False, True):
            for retain in (False, True):
                tag = 'gamma g=%g invert=%s retain_stats=%s' % (g, invert, retain)
                worst[tag] = _functional_case(dev, d, lambda x, p: color.augment_gamma_device(x, p, invert=invert, retain_stats=retain),
                                              lambda v, q, dt: IR.gamma_one(v, q, invert, retain, 1e-7, dt), g, tag)
    print('largest ratio at %s: %.3f' % (shape, max(worst.values())))
    bad = {k: v for k, v in worst.items() if not v <= 4.0}
    assert not bad, bad


def _classes(per_channel, p):
    from multitalent_amd.training.data_augmentation import color
    return {
        'brightness': (color.BrightnessMultiplicativeDevice((0.75, 1.25), per_channel=per_channel, p_per_sample=p),
                       lambda d, dt: IR.brightness(N, CN, d, dt, per_channel=per_channel, p_per_sample=p)),
        'contrast': (color.ContrastAugmentationDevice(per_channel=per_channel, p_per_sample=p),
                     lambda d, dt: IR.contrast(N, CN, d, dt, per_channel=per_channel, p_per_sample=p)),
        'gamma_inverted': (color.GammaDevice((0.7, 1.5), True, per_channel, True, p),
                           lambda d, dt: IR.gamma(N, CN, d, dt, invert_image=True, per_channel=per_channel, p_per_sample=p)),
        'gamma': (color.GammaDevice((0.7, 1.5), False, per_channel, True, p),
                  lambda d, dt: IR.gamma(N, CN, d, dt, per_channel=per_channel, p_per_sample=p)),
    }


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('per_channel', [True, False])
@pytest.mark.parametrize('kind', ['brightness', 'contrast', 'gamma_inverted', 'gamma'])
def test_classes_end_to_end(dev, kind, per_channel):
    d = _data(SHAPES[1])
    seed = 3
    obj, ref = _classes(per_channel, 1)[kind]
    x = torch.from_numpy(d.copy()).to(dev)
    np.random.seed(seed)
    assert obj(x) is x
    state = np.random.get_state()
    np.random.seed(seed)
    r64, params = ref(d, np.float64)
    assert _same_state(np.random.get_state(), state)
    np.random.seed(seed)
    r32, _ = ref(d, np.float32)
    assert not np.isnan(params).any()
    got = x.cpu().numpy()
    ratio = _ratio(got, r32, r64, d)
    print('class %s per_channel=%s: ratio %.3f' % (kind, per_channel, ratio))
    assert ratio <= 4.0
    # a non-contiguous batch: the same values through a contiguous copy
    wide = torch.zeros(N, CN, d.shape[2], d.shape[3], d.shape[4] + 3, device=dev)
    view = wide[..., :d.shape[4]]
    view.copy_(torch.from_numpy(d.copy()))
    np.random.seed(seed)
    assert obj(view) is view and not view.is_contiguous()
    assert torch.equal(view, x) and bool((wide[..., d.shape[4]:] == 0).all())
    # nothing drawn: the input comes back bit for bit
    off, _ = _classes(per_channel, 0)[kind]
    y = torch.from_numpy(d.copy()).to(dev)
    assert off(y) is y and y.cpu().numpy().tobytes() == d.tobytes()


def test_no_host_round_trip(dev):
    """With torch's synchronisation check armed (a device-to-host read raises), the four transforms of the chain run with every
    probability 1."""
    from multitalent_amd.training.data_augmentation import color
    x = torch.randn(2, 2, 5, 7, 11, device=dev)
    color.augment_brightness_device(x.clone(), np.ones((2, 2)))          # library load and device probe happen before the check is armed
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    chain = [color.BrightnessMultiplicativeDevice(p_per_sample=1.), color.ContrastAugmentationDevice(p_per_sample=1.),
             color.GammaDevice((0.7, 1.5), True, True, True, 1.), color.GammaDevice((0.7, 1.5), False, True, True, 1.)]
    np.random.seed(0)
    before = x.clone()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            armed = False
        except RuntimeError:
            armed = True
        if not armed:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
        for t in chain:
            x = t(x)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, before)


def test_cpu_tensors_are_refused(dev):
    from multitalent_amd.training.data_augmentation import color
    x = torch.zeros(2, 1, 5, 7, 11)
    for t in (color.BrightnessMultiplicativeDevice(p_per_sample=1.), color.ContrastAugmentationDevice(p_per_sample=1.),
              color.GammaDevice(p_per_sample=1.)):
        with pytest.raises(RuntimeError, match="HIP device only; there is no CPU fallback"):
            t(x)
