"""The data side on real memory against float64: mt_affine_sample, mt_warp_sample, mt_spline_prefilter3, mt_gaussian_blur_axis,
mt_gaussian_blur_axis_zero and mt_downsample_seg_nearest through the library's entry points.  Cases, references and bounds are
tests/spatial_cases.py (see its docstring); tests/test_spatial_cases_cpu.py checks the references against scipy.ndimage and shows what
the cases reach.  Every destination that is assigned starts as NaN and lies between guard elements; after a launch the guards and every
source are bit-identical and no NaN is left unless the case expects one.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import spatial_cases as SC

pytestmark = pytest.mark.gpu

IDS = lambda c: c.id
LATTICE = [c for c in SC.sample_cases() if c.kind == 'lattice']
GENERAL = [c for c in SC.sample_cases() if c.kind == 'general']


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib
    return dev, _lib.load(), _lib


def stops_on_hip_error(fn):
    """A HIP error ends the whole run: nothing more is launched on a device that has faulted (as test_infer_kernels_gpu)."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except BaseException as e:
            text = str(e)
            faulted = isinstance(e, RuntimeError) and any(s in text for s in ('rc=-3', 'HIP error', 'hipError', 'illegal memory', 'device-side'))
            if not faulted:
                try:
                    torch.cuda.synchronize()
                except Exception as e2:          # noqa: BLE001
                    faulted, text = True, str(e2)
            if faulted:
                pytest.exit('HIP error in %s: %s' % (fn.__name__, text), returncode=3)
            raise
    return run


def _fig(kernel, case_id, what, value):
    print('SPATIAL-FIG %s %s %s %.3e' % (kernel, case_id, what, value))


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


class Source(object):
    """an operand the kernel only reads: uploaded once, compared bit for bit with the host copy afterwards"""

    def __init__(self, dev, host):
        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host.copy()).to(dev)

    def ptr(self):
        return self.dev.data_ptr()

    def unchanged(self):
        return _same_bits(self.dev.cpu().numpy(), self.host)


class Guarded(object):
    """a float32 destination between SC.GUARD sentinels on each side, filled on the device: NaN, or `init` (in-place kernels)"""

    def __init__(self, dev, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.dev = torch.full((self.n + 2 * SC.GUARD,), SC.SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.dev[SC.GUARD:SC.GUARD + self.n]
        if init is None:
            self.view.fill_(float('nan'))
        else:
            self.view.copy_(torch.tensor(np.asarray(init, dtype=np.float32)).reshape(-1))

    def ptr(self):
        return self.view.data_ptr()

    def fetch(self):
        after = self.dev.cpu().numpy()
        guard = np.full(SC.GUARD, SC.SENTINEL, np.float32)
        assert _same_bits(after[:SC.GUARD], guard) and _same_bits(after[-SC.GUARD:], guard), "guard elements around a destination changed"
        return after[SC.GUARD:SC.GUARD + self.n].reshape(self.shape)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================================================
# A. the sampler
def _sample(env, c, src, mats, field=None, alpha=None, cval=None, entry=None):
    """one launch of c's entry point (mode 3: behind the library's prefilter) -> [N, C, OD, OH, OW] float32"""
    dev, lib, _lib = env
    entry = c.entry if entry is None else entry
    cval = c.cval if cval is None else cval
    D, H, W = c.in_shape
    if c.mode == 3:
        co = Guarded(dev, src.shape, init=src)
        _lib.check(lib.mt_spline_prefilter3(co.ptr(), c.N * c.C, D, H, W, 3 if c.planar else 7, _stream()), 'spline_prefilter3')
        torch.cuda.synchronize()
        s = Source(dev, co.fetch())
    else:
        s = Source(dev, src)
    ops = [s, Source(dev, mats)]
    dst = Guarded(dev, (c.N, c.C) + c.out_shape)
    if entry == 'affine':
        rc = lib.mt_affine_sample(s.ptr(), c.N, c.C, D, H, W, dst.ptr(), c.out_shape[0], c.out_shape[1], c.out_shape[2], ops[1].ptr(),
                                  c.mode, float(cval), c.planar, _stream())
    else:
        ops += [Source(dev, field), Source(dev, alpha)]
        rc = lib.mt_warp_sample(s.ptr(), c.N, c.C, D, H, W, dst.ptr(), c.out_shape[0], c.out_shape[1], c.out_shape[2], ops[1].ptr(),
                                ops[2].ptr(), ops[3].ptr(), c.mode, float(cval), c.planar, _stream())
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    got = dst.fetch()
    assert all(o.unchanged() for o in ops), "%s_sample changed a source" % entry
    assert not np.isnan(got).any(), "an output was not written"
    return got


def _unread_field(d):
    """the case's field with NaN wherever alpha is 0: such a sample's field is never read"""
    if d['field'] is None:
        return None
    f = d['field'].copy()
    f[d['alpha'] == 0] = np.nan
    return f


def _check_sample(c, d, got, ref, ins, keep=None):
    kernel = 'mt_%s_sample' % c.entry
    rng_ = float(np.ptp(d['src']))
    keep = np.ones(ins.shape, bool) if keep is None else keep
    outside = np.broadcast_to((~ins)[:, None], got.shape)
    k5 = np.broadcast_to(keep[:, None], got.shape)
    fill = 0.0 if c.mode == 11 else c.cval
    wrong_fill = int(((got == fill) != outside)[k5].sum()) if c.mode != 11 else int((got[outside & k5] != 0).sum())
    _fig(kernel, c.id, 'outputs-with-the-wrong-cval-membership', wrong_fill)
    ref32 = ref.astype(np.float32)
    if c.mode in (0, 1, 11) and (c.kind != 'general' or c.mode != 1):
        mism = int(((got + 0.0).view(np.uint32) != (ref32 + 0.0).view(np.uint32))[k5].sum())
        _fig(kernel, c.id, 'mismatching-outputs', mism)
        assert wrong_fill == 0 and mism == 0
    else:
        err = float(np.abs(got.astype(np.float64) - ref)[k5].max()) / rng_
        _fig(kernel, c.id, 'maxerr/range', err)
        assert wrong_fill == 0 and err <= SC.CUBIC_BOUND, err


@pytest.mark.parametrize('case', LATTICE, ids=IDS)
@stops_on_hip_error
def test_sampler_on_the_lattice(env, case):
    """faces, .5 ties, mirrored taps and axes of length 1: no exclusions"""
    c, d = case, SC.sample_draw(case)
    ref, ins, _ = SC.sample_case_ref(c)
    got = _sample(env, c, d['src'], d['mats'], _unread_field(d), d['alpha'])
    _check_sample(c, d, got, ref, ins)


@pytest.mark.parametrize('case', GENERAL, ids=IDS)
@stops_on_hip_error
def test_sampler_in_general_position(env, case):
    c, d = case, SC.sample_draw(case)
    ref, ins, coords = SC.sample_case_ref(c)
    ex = SC.general_exclusions(c, d, coords)
    _fig('mt_%s_sample' % c.entry, c.id, 'excluded-share', ex.mean())
    assert ex.mean() <= SC.EXCLUDE_CAP
    got = _sample(env, c, d['src'], d['mats'], _unread_field(d), d['alpha'])
    _check_sample(c, d, got, ref, ins, ~ex)


NONFINITE = [c for c in LATTICE if c.in_shape == (2, 3, 5)]
# slots that planar sampling reads as well; 1e30 goes into the centre because a matrix entry is multiplied by a mesh coordinate that is 0 somewhere
POISON = (('nan-matrix', 4, float('nan')), ('inf-matrix', 8, float('inf')), ('1e30-centre', 11, 1e30), ('-inf-centre', 10, float('-inf')))


@pytest.mark.parametrize('case', NONFINITE, ids=IDS)
@stops_on_hip_error
def test_sampler_non_finite_coordinates_give_cval(env, case):
    """sample 1 gets a NaN, an infinity or 1e30 into its matrix / centre (mt_warp_sample: also a NaN field): all of its outputs are cval
    (mode 11: 0) and the other samples keep their bits — the range check is made in double before any integer conversion"""
    c, d = case, SC.sample_draw(case)
    kernel = 'mt_%s_sample' % c.entry
    field = _unread_field(d)
    clean = _sample(env, c, d['src'], d['mats'], field, d['alpha'])
    fill = np.float32(0.0 if c.mode == 11 else c.cval)
    for name, slot, value in POISON:
        mats = d['mats'].copy()
        mats[1, slot] = value
        got = _sample(env, c, d['src'], mats, field, d['alpha'])
        bad = int((got[1] != fill).sum())
        moved = int(not _same_bits(got[[0, 2]], clean[[0, 2]]))
        _fig(kernel, c.id, name + '-outputs-not-cval', bad)
        _fig(kernel, c.id, name + '-other-samples-changed', moved)
        assert bad == 0 and moved == 0
    if c.entry == 'warp':
        f2 = field.copy()
        f2[1] = np.nan                                         # alpha[1] = 8: the displaced coordinate is NaN everywhere
        f2[0, 0].reshape(-1)[::5] = np.nan                     # and in every 5th element of sample 0's first component (alpha 4)
        got = _sample(env, c, d['src'], d['mats'], f2, d['alpha'])
        comp0 = np.isnan(f2[0, 0])
        hit = np.broadcast_to(comp0[None] if c.planar else comp0, c.out_shape)
        bad = int((got[1] != fill).sum()) + int((got[0][:, hit] != fill).sum())
        moved = int(not _same_bits(got[2], clean[2])) + int(not _same_bits(got[0][:, ~hit], clean[0][:, ~hit]))
        _fig(kernel, c.id, 'nan-field-outputs-not-cval', bad)
        _fig(kernel, c.id, 'nan-field-other-outputs-changed', moved)
        assert bad == 0 and moved == 0
        # alpha == 0 with a NaN field: mt_affine_sample's bits
        aff = _sample(env, c, d['src'], d['mats'], entry='affine')
        same = int(_same_bits(aff[2], clean[2]))
        _fig(kernel, c.id, 'alpha0-is-affine', same)
        assert same == 1


@pytest.mark.parametrize('case', SC.stride_cases(), ids=IDS)
@stops_on_hip_error
def test_sampler_grid_stride(env, case):
    """more outputs than 65536 blocks x 256 threads: the loop's second trip"""
    c, d = case, SC.sample_draw(case)
    got = _sample(env, c, d['src'], d['mats'], d['field'], d['alpha'])
    ref = SC.stride_ref(c)
    first = SC.CAP_SAMPLE * SC.BLOCK
    mism = (got + 0.0).reshape(-1).view(np.uint32) != (ref + 0.0).reshape(-1).view(np.uint32)
    _fig('mt_%s_sample' % c.entry, c.id, 'mismatching-outputs-first-trip', int(mism[:first].sum()))
    _fig('mt_%s_sample' % c.entry, c.id, 'mismatching-outputs-second-trip', int(mism[first:].sum()))
    _fig('mt_%s_sample' % c.entry, c.id, 'inside-outputs-second-trip', int((ref.reshape(-1)[first:] != np.float32(c.cval)).sum()))
    assert not mism.any() and (ref.reshape(-1)[first:] != np.float32(c.cval)).any()


@stops_on_hip_error
def test_label_rule_with_cval_below_half_and_its_refusal(env):
    """cval = 0.49 is still the reference's rule (no indicator reaches 0.5 outside the volume); from 0.5 on it is refused"""
    from multitalent_amd.training.data_augmentation.spatial import affine_sample, warp_sample
    dev = env[0]
    for c in LATTICE:
        if c.mode == 11 and c.in_shape == (4, 5, 6):
            d = SC.sample_draw(c)
            ref, ins, _ = SC.sample_case_ref(c)
            x, args = torch.tensor(d['src']).to(dev), (d['mats'], c.out_shape, 1)
            if c.entry == 'affine':
                call = lambda cv: affine_sample(x, *args, cval=cv, is_seg=True, planar=bool(c.planar))
            else:
                fld, al = torch.tensor(d['field']).to(dev), d['alpha']
                call = lambda cv: warp_sample(x, *args, fld, al, cval=cv, is_seg=True, planar=bool(c.planar))
            got = call(0.49).cpu().numpy()
            mism = int((got != ref.astype(np.float32)).sum())
            _fig('mt_%s_sample' % c.entry, c.id, 'cval0.49-mismatching-outputs', mism)
            assert mism == 0 and (got[np.broadcast_to((~ins)[:, None], got.shape)] == 0).all()
            for cv in (0.5, 2.0):
                with pytest.raises(NotImplementedError, match='largest label'):
                    call(cv)


# ================================================================================================================================
# B. mt_spline_prefilter3
def _prefilter(env, c, x, axes):
    dev, lib, _lib = env
    buf = Guarded(dev, x.shape, init=x)
    _lib.check(lib.mt_spline_prefilter3(buf.ptr(), c.NC, c.shape[0], c.shape[1], c.shape[2], axes, _stream()), 'spline_prefilter3')
    torch.cuda.synchronize()
    got = buf.fetch()
    assert not np.isnan(got).any()
    return got


@pytest.mark.parametrize('case', SC.prefilter_cases(), ids=IDS)
@stops_on_hip_error
def test_spline_prefilter(env, case):
    """Every pass within 2^-23 |ref| + 1e-12 max|line| of spline_filter1d ON THE SAME float32 INPUT.  A call over several axes is
    checked pass by pass — the call's result is bit-identical to the kernel's own single-axis calls in the order W, H, D, and each of
    those is compared with scipy's pass over the array the kernel's pass read.  The bound cannot hold for the free-running composition
    (scipy's passes chained on scipy's own float32 results): where the two double results of a pass straddle a float32 rounding
    boundary, one element differs by an ulp, and the next pass spreads that over the element's line, beyond 2^-23 of a small
    neighbour.  Measured on an MI355X: pf-a3-* 0 (bit-identical), pf-a7-11x9x10 3.6 x the bound (4.8e-9 of max|ref|), pf-a7-280x10x9
    22.7 x (5.5e-8 of max|ref|); that figure is printed, the per-pass figures are asserted."""
    c, x = case, SC.prefilter_draw(case)
    got = _prefilter(env, c, x, c.axes)
    bits = [b for b in (1, 2, 4) if c.axes & b]
    cur, worst = x, 0.0
    for b in bits:
        step = got if len(bits) == 1 else _prefilter(env, c, cur, b)
        ref, linemax = SC.prefilter_ref(c._replace(axes=b), cur)
        diff = np.abs(step.astype(np.float64) - ref.astype(np.float64))
        ratio = float((diff / SC.prefilter_bound(ref, linemax)).max())
        _fig('mt_spline_prefilter3', c.id, 'pass%d-max-diff/bound' % b, ratio)
        _fig('mt_spline_prefilter3', c.id, 'pass%d-max-diff/max-ref' % b, float(diff.max() / np.abs(ref).max()))
        worst, cur = max(worst, ratio), step
    if len(bits) > 1:
        ref, linemax = SC.prefilter_ref(c, x)
        diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        _fig('mt_spline_prefilter3', c.id, 'free-running-max-diff/bound', float((diff / SC.prefilter_bound(ref, linemax)).max()))
        same = int(_same_bits(got, cur))
        _fig('mt_spline_prefilter3', c.id, 'one-call-is-its-passes', same)
        assert same == 1
    if all(c.shape[SC.PF_AXIS[b]] == 1 for b in bits):
        same = int(_same_bits(got, x))
        _fig('mt_spline_prefilter3', c.id, 'length-1-bits-kept', same)
        assert same == 1
    assert worst <= 1.0


# ================================================================================================================================
# C. mt_gaussian_blur_axis
def _reflect_blur(env, shape, axis, x, sigmas):
    dev, lib, _lib = env
    src, sg = Source(dev, x), Source(dev, np.asarray(sigmas, np.float32))
    dst = Guarded(dev, x.shape)
    _lib.check(lib.mt_gaussian_blur_axis(src.ptr(), dst.ptr(), len(sigmas), shape[0], shape[1], shape[2], axis, sg.ptr(), _stream()),
               'gaussian_blur_axis')
    torch.cuda.synchronize()
    got = dst.fetch()
    assert src.unchanged() and sg.unchanged(), "gaussian_blur_axis changed a source"
    return got


@pytest.mark.parametrize('case', SC.reflect_blur_cases(), ids=IDS)
@stops_on_hip_error
def test_reflect_blur_one_axis(env, case):
    c, x = case, SC.blur_draw(case)
    got = _reflect_blur(env, c.shape, c.axis, x, c.sigmas)
    assert not np.isnan(got).any()
    ref = SC.blur_ref(c, x, 'reflect')
    for ch, sg in enumerate(c.sigmas):
        if sg <= 0:
            same = int(_same_bits(got[ch], x[ch]))
            _fig('mt_gaussian_blur_axis', c.id, 'ch%d-sigma%g-copy-bits-kept' % (ch, sg), same)
            assert same == 1
        else:
            err = float(np.abs(got[ch].astype(np.float64) - ref[ch]).max() / np.abs(x[ch]).max())
            _fig('mt_gaussian_blur_axis', c.id, 'ch%d-r%d-maxerr/max-src' % (ch, SC.radius(sg)), err)
            assert err <= 2.0 ** -22, (ch, sg, err)


@stops_on_hip_error
def test_reflect_blur_never_clamps_a_radius(env):
    """a sigma whose radius exceeds 32, or a NaN: the kernel cannot refuse a device sigma, so the channel is NaN throughout; the wrapper
    and the transform refuse on the host.  (A clamped radius is a different filter: at sigma 8.2 / 9 / 13 it is off by 1.5e-4 / 7.2e-4 /
    2.6e-2 of the output's maximum.)"""
    from multitalent_amd.training.data_augmentation.color import GaussianBlurDevice, gaussian_filter_device
    dev = env[0]
    sig = (1.0,) + SC.RB_REFUSED + (0.0, 8.0)
    for axis, shape in enumerate(((19, 5, 6), (5, 19, 6), (3, 2, 300))):
        c = SC.BlurCase('rb-refused-ax%d' % axis, shape, axis, sig)
        x = SC.blur_draw(c)
        got = _reflect_blur(env, shape, axis, x, sig)
        ref = SC.blur_ref(SC.BlurCase(c.id, shape, axis, tuple(s if (s == s and s < 8.1) else 0.0 for s in sig)), x, 'reflect')
        for ch, sg in enumerate(sig):
            if sg in SC.RB_REFUSED or sg != sg:
                finite = int((~np.isnan(got[ch])).sum())
                _fig('mt_gaussian_blur_axis', c.id, 'ch%d-sigma%g-elements-not-NaN' % (ch, sg), finite)
                assert finite == 0
            else:
                err = float(np.abs(got[ch].astype(np.float64) - ref[ch]).max() / np.abs(x[ch]).max())
                _fig('mt_gaussian_blur_axis', c.id, 'ch%d-sigma%g-maxerr/max-src' % (ch, sg), err)
                assert err <= 2.0 ** -22
    x = torch.tensor(SC.blur_draw(SC.BlurCase('rb-wrapper', (7, 9, 11), 0, (1.0, 2.0)))[None]).to(dev)
    for bad in SC.RB_REFUSED:
        with pytest.raises(ValueError, match='radius above 32'):
            gaussian_filter_device(x, np.array([[1.0, bad]], np.float32))
        with pytest.raises(ValueError, match='radius above 32'):
            GaussianBlurDevice(blur_sigma=(0.5, bad))
    out = gaussian_filter_device(x, np.array([[8.0, 0.0]], np.float32)).cpu().numpy()
    ref = ndimage.gaussian_filter(x[0, 0].cpu().numpy().astype(np.float64), 8.0)
    err = float(np.abs(out[0, 0] - ref).max() / np.abs(x.cpu().numpy()).max())
    _fig('gaussian_filter_device', 'sigma8-r32', 'maxerr/max-src', err)
    assert err <= 2e-6 and _same_bits(out[0, 1], x[0, 1].cpu().numpy())


# ================================================================================================================================
# D. mt_gaussian_blur_axis_zero
def _zero_blur(env, shape, axis, x, sigmas, expect_rc0=True):
    dev, lib, _lib = env
    src = Source(dev, x)
    sg = np.ascontiguousarray(np.asarray(sigmas, np.float32))
    sg0 = sg.copy()
    dst = Guarded(dev, x.shape)
    rc = lib.mt_gaussian_blur_axis_zero(src.ptr(), dst.ptr(), len(sigmas), shape[0], shape[1], shape[2], axis,
                                        sg.ctypes.data_as(_lib.c_float_p), _stream())
    if expect_rc0:
        _lib.check(rc, 'gaussian_blur_axis_zero')
    torch.cuda.synchronize()
    got = dst.fetch()
    assert src.unchanged() and _same_bits(sg, sg0), "gaussian_blur_axis_zero changed a source"
    return got, rc


@pytest.mark.parametrize('case', SC.zero_blur_cases(), ids=IDS)
@stops_on_hip_error
def test_zero_blur_one_axis(env, case):
    c, x = case, SC.blur_draw(case)
    got, _ = _zero_blur(env, c.shape, c.axis, x, c.sigmas)
    assert not np.isnan(got).any()
    ref = SC.blur_ref(c, x, 'constant')
    worst, copies = 0.0, 0
    for ch, sg in enumerate(c.sigmas):
        if sg <= 0:
            copies += int(not _same_bits(got[ch], x[ch]))
        else:
            ratio = float((np.abs(got[ch].astype(np.float64) - ref[ch]) / SC.zero_blur_bound(ref[ch], x[ch])).max())
            if len(c.sigmas) <= 8:
                _fig('mt_gaussian_blur_axis_zero', c.id, 'ch%d-r%d-max-diff/bound' % (ch, SC.radius(sg)), ratio)
            worst = max(worst, ratio)
    _fig('mt_gaussian_blur_axis_zero', c.id, 'worst-diff/bound', worst)
    _fig('mt_gaussian_blur_axis_zero', c.id, 'copied-channels-with-changed-bits', copies)
    assert worst <= 1.0 and copies == 0


@stops_on_hip_error
def test_zero_blur_refusals_and_three_passes(env):
    from multitalent_amd.training.data_augmentation.spatial import gaussian_filter_zero_device
    dev = env[0]
    c = SC.ZeroCase('zb-refused', (3, 5, 7), 1, (1.0, 16.2, 0.0), 'randn')
    x = SC.blur_draw(c)
    for bad in (16.2, 16.125, float('nan')):
        got, rc = _zero_blur(env, c.shape, c.axis, x, (1.0, bad, 0.0), expect_rc0=False)
        _fig('mt_gaussian_blur_axis_zero', c.id, 'sigma%g-rc' % bad, rc)
        assert rc != 0 and np.isnan(got).all()                  # refused before anything is launched
        with pytest.raises(ValueError):
            gaussian_filter_zero_device(torch.tensor(x[None]).to(dev), np.array([[1.0, bad, 0.0]], np.float32))
    r = SC.rng('zb-three')
    x = r.randn(1, 4, 13, 67, 70).astype(np.float32)
    sg = np.array([[0.7, 0.0, 2.2, 15.9]], np.float32)
    t = torch.from_numpy(x).to(dev)
    got = gaussian_filter_zero_device(t, sg).cpu().numpy()
    assert _same_bits(t.cpu().numpy(), x)
    for ch in range(4):
        if sg[0, ch] <= 0:
            assert _same_bits(got[0, ch], x[0, ch])
            continue
        ref = ndimage.gaussian_filter(x[0, ch].astype(np.float64), float(sg[0, ch]), mode='constant', cval=0.0)
        err = float(np.abs(got[0, ch] - ref).max() / np.ptp(ref))
        _fig('gaussian_filter_zero_device', 'three-passes', 'ch%d-maxerr/range' % ch, err)
        assert err <= 2e-6


# ================================================================================================================================
# E. mt_downsample_seg_nearest
@pytest.mark.parametrize('remove', [0, 1], ids=['keep', 'remove-1'])
@pytest.mark.parametrize('case', SC.pyramid_cases(), ids=IDS)
@stops_on_hip_error
def test_label_pyramid(env, case, remove):
    dev, lib, _lib = env
    c, x = case, SC.pyramid_draw(case)
    src = Source(dev, x)
    dst = Guarded(dev, (c.NC,) + c.out_shape)
    _lib.check(lib.mt_downsample_seg_nearest(src.ptr(), c.NC, c.in_shape[0], c.in_shape[1], c.in_shape[2], dst.ptr(), c.out_shape[0],
                                             c.out_shape[1], c.out_shape[2], remove, _stream()), 'downsample_seg_nearest')
    torch.cuda.synchronize()
    got = dst.fetch()
    assert src.unchanged() and not np.isnan(got).any()
    ref = SC.pyramid_ref(c, x, remove)
    mism = int((_bits(got) != _bits(ref)).sum())
    _fig('mt_downsample_seg_nearest', c.id + ('-remove' if remove else ''), 'mismatching-outputs', mism)
    assert mism == 0 and bool((ref == -1.0).any()) == (not remove)
