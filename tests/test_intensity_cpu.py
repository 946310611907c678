"""Host half of the intensity augmentation (training/data_augmentation/color.py), no GPU: `plan` of BrightnessMultiplicativeDevice,
ContrastAugmentationDevice and GammaDevice makes all draws of a batch in the order of the per-(sample, channel) loops they replaced
(tests/intensity_restatement.py): same parameters, same numpy random state afterwards.  The new C symbols are bound with the
header's argument counts, the op record has the C layout, and an oversized channel is refused before anything is launched."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intensity_restatement as IR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _pairs(per_channel, p):
    from multitalent_amd.training.data_augmentation import color
    return {
        'brightness': (color.BrightnessMultiplicativeDevice((0.75, 1.25), per_channel=per_channel, p_per_sample=p),
                       lambda N, Cn: IR.brightness(N, Cn, multiplier_range=(0.75, 1.25), per_channel=per_channel, p_per_sample=p)),
        'contrast': (color.ContrastAugmentationDevice((0.75, 1.25), per_channel=per_channel, p_per_sample=p),
                     lambda N, Cn: IR.contrast(N, Cn, contrast_range=(0.75, 1.25), per_channel=per_channel, p_per_sample=p)),
        'gamma': (color.GammaDevice((0.7, 1.5), True, per_channel, True, p),
                  lambda N, Cn: IR.gamma(N, Cn, gamma_range=(0.7, 1.5), invert_image=True, per_channel=per_channel, p_per_sample=p)),
    }


@pytest.mark.parametrize('kind', ['brightness', 'contrast', 'gamma'])
@pytest.mark.parametrize('per_channel', [True, False])
@pytest.mark.parametrize('p', [0, 0.3, 1])
def test_plan_makes_the_draws_of_the_loops_it_replaces(kind, per_channel, p):
    obj, ref = _pairs(per_channel, p)[kind]
    drawn = 0
    for seed in range(10):
        for N, Cn in ((2, 1), (3, 4)):
            np.random.seed(seed)
            _, want = ref(N, Cn)
            state = np.random.get_state()
            np.random.seed(seed)
            got = obj.plan(N, Cn)
            assert _same_state(np.random.get_state(), state), (kind, seed, N, Cn)
            assert got.shape == (N, Cn if per_channel else 1) and got.dtype == np.float64
            assert np.array_equal(np.broadcast_to(got, (N, Cn)), want, equal_nan=True), (kind, seed, N, Cn)
            drawn += int((~np.isnan(got)).sum())
    if p == 0:
        assert drawn == 0
    elif p == 1:
        assert drawn == 10 * ((2 * 1 + 3 * 4) if per_channel else (2 + 3))
    else:
        assert 0 < drawn < 10 * ((2 * 1 + 3 * 4) if per_channel else (2 + 3))


def _header():
    txt = open(os.path.join(ROOT, 'include', 'mtseg.h')).read()
    return re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


def test_new_symbols_are_bound_with_the_headers_argument_counts():
    from multitalent_amd import _lib
    txt = _header()
    for name in ('mt_channel_stats_workspace', 'mt_channel_stats', 'mt_intensity_apply'):
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, txt)
        assert m, name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(',')), name
    assert _lib.SIGNATURES['mt_channel_stats_workspace'][0] is C.c_size_t


def test_op_record_has_the_c_layout_and_the_headers_codes():
    from multitalent_amd import _lib, ops
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mtseg.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", '
           'sizeof(mt_intensity_op_t), offsetof(mt_intensity_op_t, op), offsetof(mt_intensity_op_t, flags), offsetof(mt_intensity_op_t, a), '
           'offsetof(mt_intensity_op_t, b), MT_INTENSITY_NONE, MT_INTENSITY_SCALE, MT_INTENSITY_CONTRAST, MT_INTENSITY_GAMMA, '
           'MT_INTENSITY_RESTORE, MT_INTENSITY_PRESERVE_RANGE, MT_INTENSITY_NEGATE);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).decode().split()]
    T, dt = _lib.mt_intensity_op_t, ops.INTENSITY_OP_DTYPE
    assert out[:5] == [C.sizeof(T), T.op.offset, T.flags.offset, T.a.offset, T.b.offset]
    assert out[:5] == [dt.itemsize] + [dt.fields[k][1] for k in ('op', 'flags', 'a', 'b')]
    assert out[5:] == [ops.INTENSITY_NONE, ops.INTENSITY_SCALE, ops.INTENSITY_CONTRAST, ops.INTENSITY_GAMMA, ops.INTENSITY_RESTORE,
                       ops.INTENSITY_PRESERVE_RANGE, ops.INTENSITY_NEGATE]


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks are host code and come before every launch: a channel beyond the int32 index range, an unknown op and a
    record without its statistics return MT_EINVAL (-1) with a message.  The pointers are never dereferenced."""
    from multitalent_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.float64)
    ptr = C.c_void_p(buf.ctypes.data)
    big = 2 ** 31
    assert lib.mt_channel_stats_workspace(1, big) == 0
    assert lib.mt_channel_stats(ptr, 1, big, None, ptr, ptr, 1 << 40, None) == -1
    assert b'int32' in lib.mt_last_error()
    rec = (_lib.mt_intensity_op_t * 1)()
    rec[0].op = _lib.MT_INTENSITY_SCALE
    assert lib.mt_intensity_apply(ptr, 1, big, rec, None, None, None) == -1
    assert b'int32' in lib.mt_last_error()
    rec[0].op = 7
    assert lib.mt_intensity_apply(ptr, 1, 16, rec, None, None, None) == -1
    assert b'unknown op' in lib.mt_last_error()
    rec[0].op = _lib.MT_INTENSITY_GAMMA
    assert lib.mt_intensity_apply(ptr, 1, 16, rec, None, None, None) == -1
    rec[0].op = _lib.MT_INTENSITY_RESTORE
    assert lib.mt_intensity_apply(ptr, 1, 16, rec, ptr, None, None) == -1
    assert b'second statistics' in lib.mt_last_error()


def test_functional_forms_refuse_cpu_tensors():
    import torch
    from multitalent_amd.training.data_augmentation import color
    x = torch.zeros(1, 1, 2, 3, 4)
    one = np.ones((1, 1))
    for call in (lambda: color.augment_brightness_device(x, one), lambda: color.augment_contrast_device(x, one),
                 lambda: color.augment_gamma_device(x, one), lambda: color.GammaDevice(p_per_sample=0.)(x)):
        with pytest.raises(RuntimeError, match="HIP device only; there is no CPU fallback"):
            call()
