"""The resize unit on the device.  The kernel entries alone against the float64 restatement (tests/resampling_cases.py, which
tests/test_resampling_cases_cpu.py ties to scipy.ndimage itself): order 0 and the label passes exact, orders 1 and 3 within the
bounds below, destinations between guard elements, in place and out of place, every axis as the anisotropic one, two runs identical
bit for bit, every refusal without a launch.  The Python functions and both preprocessors against the REAL reference
(tests/golden/resampling.npz, tools/oracle_gen/make_golden_resampling.py).  One chain at toy size through
`nnUNet_plan_and_preprocess -pl3d ExperimentPlanner3D_v23` into `preprocess_patient`.

Bounds.  Data against the float64 result of scipy's arithmetic: 2e-4 after the "CT" scheme with the intensity properties of
tests/test_preprocess_gpu.py (sd 175.48), which is the bound that file holds the existing order-3 path to; for raw volumes the same
times the sd, 0.035.  The per-case schemes add twice the reference's own recorded deviation between float32 and float64 moments, as
tests/test_train_preprocess_gpu.py does.  A kernel against the restatement of that kernel is held tighter, from the number formats:
the prefilter within 2^-21 of the largest coefficient per pass (one rounding to float32, 2^-24; the device rebuilds the causal values
of a chunk from 40 inputs, 1e-23; what is left covers a last-bit difference carried through the later passes), the sampler on the
device's own coefficients within 2^-22 of the largest coefficient (one rounding of the result plus the double sums).  Labels are
compared outside the golden's fragile voxels, which leave at least 0.90 of every case.  Every figure is printed before it is asserted.
Measured on an MI355X: see DESIGN section 6af."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planning_cases as PC  # noqa: E402
import resampling_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resampling.npz')
GUARD, SENTINEL = 64, -7.25e9
RAW_BOUND, CT_BOUND = 0.035, 2e-4
GEOMS = ['up', 'double', 'mixed', 'iso_down', 'axis_last', 'z_same']
DATA_ORDERS = [(1, 0), (3, 3), (3, 1), (0, 0)]
SEG_ORDERS = [(1, 1), (1, 0), (0, 0)]
CASES = ['diff_up_ct', 'diff_mixed_ct2_mask', 'diff_axis_last_zscore_nonorm', 'diff_iso_down_ct_mask', 'lin_up_ct',
         'lin_iso_down_zscore_mask', 'lin_z_same_ct2']


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib
    return dev, _lib.load(), _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Guarded(object):
    """a float32 destination between GUARD sentinels on each side: NaN, or `init` (in-place kernels)"""

    def __init__(self, dev, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.dev = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.dev[GUARD:GUARD + self.n]
        if init is None:
            self.view.fill_(float('nan'))
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).reshape(-1))

    def ptr(self):
        return self.view.data_ptr()

    def fetch(self):
        after = self.dev.cpu().numpy()
        guard = np.full(GUARD, SENTINEL, np.float32)
        assert np.array_equal(_bits(after[:GUARD]), _bits(guard)) and np.array_equal(_bits(after[-GUARD:]), _bits(guard)), \
            "guard elements around a destination changed"
        return after[GUARD:GUARD + self.n].reshape(self.shape)


def _prefilter(env, x, axes, in_place):
    dev, lib, _lib = env
    NC, D, H, W = x.shape
    if in_place:
        buf = Guarded(dev, x.shape, init=x)
        _lib.check(lib.mt_resize_prefilter3(buf.ptr(), buf.ptr(), NC, D, H, W, axes, _stream()), 'resize_prefilter3')
        return buf.fetch()
    src = torch.from_numpy(x.copy()).to(dev)
    buf = Guarded(dev, x.shape)
    _lib.check(lib.mt_resize_prefilter3(src.data_ptr(), buf.ptr(), NC, D, H, W, axes, _stream()), 'resize_prefilter3')
    out = buf.fetch()
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(x)), "the source changed"
    return out


def _resize(env, x, out_shape, orders):
    dev, lib, _lib = env
    NC, D, H, W = x.shape
    src = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    buf = Guarded(dev, (NC,) + tuple(out_shape))
    _lib.check(lib.mt_resize(src.data_ptr(), NC, D, H, W, buf.ptr(), *out_shape, *orders, _stream()), 'resize')
    out = buf.fetch()
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(np.ascontiguousarray(x, dtype=np.float32))), "the source changed"
    return out


def _mask(x, out_shape, orders):
    return sum(1 << (2 - a) for a in range(3) if orders[a] == 3 and x.shape[1 + a] != out_shape[a])


# ---- A. the kernel entries against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RC.VOLUME_CASES, ids=lambda c: c[0])
def test_resize_against_the_restatement(env, case):
    name, shape, out_shape, orders = case
    x = RC.hu_volume(shape, 7 + len(name), nc=1 if name == 'large' else 2)
    axes = _mask(x, out_shape, orders)
    coef = x
    if axes:
        coef = _prefilter(env, x, axes, in_place=False)
        ref_c = RC.prefilter(x, axes)
        dc, bound = float(np.abs(coef.astype(np.float64) - ref_c).max()), bin(axes).count('1') * 2.0 ** -21 * float(np.abs(ref_c).max())
        print('RESIZE-FIG %s prefilter max |device - restatement| %.3e bound %.3e (largest coefficient %.1f)' % (name, dc, bound, np.abs(ref_c).max()))
        assert not np.isnan(coef).any() and dc <= bound
        assert np.array_equal(_bits(coef), _bits(_prefilter(env, x, axes, in_place=True))), "in place differs from out of place"
    got = _resize(env, coef, out_shape, orders)
    assert got.shape == (x.shape[0],) + tuple(out_shape) and not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(_resize(env, coef, out_shape, orders))), "two runs differ"
    own = RC.resize(coef, out_shape, orders)                      # the sampler alone: on the device's own coefficients
    d_own, b_own = float(np.abs(got - own).max()), 2.0 ** -22 * float(np.abs(coef).max())
    print('RESIZE-FIG %s sampler max |device - restatement| %.3e bound %.3e' % (name, d_own, b_own))
    if all(o == 0 or a == b for o, a, b in zip(orders, shape, out_shape)):
        assert np.array_equal(got.astype(np.float64), own), "order 0 / unchanged axes copy elements"
    assert d_own <= b_own
    exact = RC.resize_data(x, out_shape, orders, store=np.float64)          # scipy's arithmetic in float64
    d64 = float(np.abs(got - exact).max())
    print('RESIZE-FIG %s max |device - float64| %.3e (raw bound %.3e)' % (name, d64, RAW_BOUND))
    assert d64 <= RAW_BOUND


def test_order_0_takes_scipys_neighbour_at_ties(env):
    """in/out = 4/3: every third coordinate lies exactly between two elements; a fused multiply-add in the coordinate would differ."""
    x = RC.hu_volume((24, 8, 12), 3)
    for out_shape in ((18, 8, 12), (18, 6, 9), (24, 8, 9)):
        got = _resize(env, x, out_shape, (0, 0, 0))
        assert np.array_equal(got.astype(np.float64), RC.resize(x, out_shape, (0, 0, 0))), out_shape
    ties = sum(abs(float(RC.coord(o, 24, 18)) + 0.5 - round(float(RC.coord(o, 24, 18)) + 0.5)) < 1e-12 for o in range(18))
    assert ties == 6


@pytest.mark.parametrize('shape', [(2, 5, 33, 7), (1, 1, 45, 1), (3, 2, 1, 90), (1, 70, 3, 2)], ids=str)
def test_prefilter_every_axis_subset_in_place_and_out_of_place(env, shape):
    """Lines of length 1 are copied; lines longer than one chunk of 32 (33, 45, 70, 90) rebuild their causal values."""
    x = RC.hu_volume(shape[1:], 11, nc=shape[0])
    for axes in range(1, 8):
        ref = RC.prefilter(x, axes)
        out = _prefilter(env, x, axes, in_place=False)
        inp = _prefilter(env, x, axes, in_place=True)
        bound = bin(axes).count('1') * 2.0 ** -21 * float(np.abs(ref).max())
        d = float(np.abs(out.astype(np.float64) - ref).max())
        print('RESIZE-FIG prefilter %s axes %d max |device - restatement| %.3e bound %.3e' % (shape, axes, d, bound))
        assert np.array_equal(_bits(out), _bits(inp)) and not np.isnan(out).any() and d <= bound
        for bit, ax in ((0, 3), (1, 2), (2, 1)):
            if shape[ax] == 1 and axes == 1 << bit:
                assert np.array_equal(_bits(out), _bits(x)), "a line of length 1 is copied"


LABEL_CASES = [('plane_axis0', (7, 12, 11), (7, 17, 9)), ('plane_axis1', (12, 7, 11), (17, 7, 9)), ('plane_axis2', (12, 11, 7), (17, 9, 7)),
               ('volume_up', (5, 12, 12), (10, 24, 24)), ('volume_down', (12, 13, 11), (7, 8, 6)), ('one_axis', (6, 5, 9), (6, 5, 31))]


@pytest.mark.parametrize('case', LABEL_CASES, ids=lambda c: c[0])
def test_label_resize_is_exact(env, case):
    dev, lib, _lib = env
    name, shape, out_shape = case
    seg = RC.blocky_labels(shape, 5 + len(name), nc=2)
    src = torch.from_numpy(seg).to(dev)
    runs = []
    for _ in range(2):
        buf = Guarded(dev, (2,) + out_shape)
        _lib.check(lib.mt_resize_labels(src.data_ptr(), 2, *shape, buf.ptr(), *out_shape, _stream()), 'resize_labels')
        runs.append(buf.fetch())
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(src.cpu().numpy()), _bits(seg))
    ref = RC.resize_labels(seg, out_shape)
    print('RESIZE-FIG labels %s mismatches %d of %d, labels %s' % (name, int((runs[0] != ref).sum()), ref.size, np.unique(runs[0])))
    assert np.array_equal(runs[0].astype(np.float64), ref) and -1.0 in runs[0]


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_label_z_pass_is_exact(env, axis):
    """Doubling puts weights of exactly one half on every output element of the axis' interior: there no label wins and the result is
    0, unless both taps carry the same label."""
    dev, lib, _lib = env
    shape = [11, 12, 13]
    shape[axis] = 7
    seg = RC.blocky_labels(tuple(shape), 20 + axis, nc=2)
    src = torch.from_numpy(seg).to(dev)
    for out_n in (14, 4, 21, 7, 1):
        oshape = list(shape)
        oshape[axis] = out_n
        runs = []
        for _ in range(2):
            buf = Guarded(dev, [2] + oshape)
            _lib.check(lib.mt_resize_labels_axis(src.data_ptr(), 2, *shape, axis, out_n, buf.ptr(), _stream()), 'resize_labels_axis')
            runs.append(buf.fetch())
        ref = RC.resize_labels_axis(seg, axis, out_n)
        assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
        assert np.array_equal(runs[0].astype(np.float64), ref), (axis, out_n, int((runs[0] != ref).sum()))
        if out_n == 7:
            assert np.array_equal(_bits(runs[0]), _bits(seg))
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(seg))


def test_refusals_leave_the_destination_alone(env):
    dev, lib, _lib = env
    src = torch.zeros(64, device=dev)
    buf = Guarded(dev, (64,))
    s, d, st = src.data_ptr(), buf.ptr(), _stream()
    bad = [lib.mt_resize_prefilter3(None, d, 1, 2, 2, 2, 7, st), lib.mt_resize_prefilter3(s, None, 1, 2, 2, 2, 7, st),
           lib.mt_resize_prefilter3(s, d, 1, 0, 2, 2, 7, st), lib.mt_resize_prefilter3(s, d, 1, 2, 2, 2, 0, st),
           lib.mt_resize_prefilter3(s, d, 1, 2, 2, 2, 8, st), lib.mt_resize_prefilter3(s, d, 1 << 16, 1 << 15, 1, 1, 1, st),
           lib.mt_resize(None, 1, 2, 2, 2, d, 2, 2, 2, 1, 1, 1, st), lib.mt_resize(s, 1, 2, 2, 2, None, 2, 2, 2, 1, 1, 1, st),
           lib.mt_resize(s, 1, 2, -1, 2, d, 2, 2, 2, 1, 1, 1, st), lib.mt_resize(s, 1, 2, 2, 2, d, 2, 0, 2, 1, 1, 1, st),
           lib.mt_resize(s, 1, 2, 2, 2, d, 2, 2, 2, 2, 1, 1, st), lib.mt_resize(s, 1, 2, 2, 2, d, 2, 2, 2, 1, 4, 1, st),
           lib.mt_resize(s, 1, 2, 2, 2, d, 2, 2, 2, 1, 1, -3, st), lib.mt_resize(s, 1 << 16, 1 << 15, 1, 1, d, 1, 1, 1, 0, 0, 0, st),
           lib.mt_resize(s, 1, 1, 1, 1, d, 1 << 11, 1 << 10, 1 << 10, 0, 0, 0, st),
           lib.mt_resize_labels(None, 1, 2, 2, 2, d, 2, 2, 2, st), lib.mt_resize_labels(s, 0, 2, 2, 2, d, 2, 2, 2, st),
           lib.mt_resize_labels(s, 1, 1, 1, 1, d, 1 << 11, 1 << 10, 1 << 10, st),
           lib.mt_resize_labels_axis(s, 1, 2, 2, 2, 3, 4, d, st), lib.mt_resize_labels_axis(s, 1, 2, 2, 2, 0, 0, d, st),
           lib.mt_resize_labels_axis(s, 1, 2, 2, 2, 0, 4, None, st), lib.mt_resize_labels_axis(s, 1, 2, 1 << 15, 1 << 15, 0, 4, d, st)]
    assert bad == [-1] * len(bad)
    assert np.isnan(buf.fetch()).all()
    from multitalent_amd import ops
    from multitalent_amd.preprocessing import device_preprocessing as dp
    x = torch.zeros(1, 4, 4, 4, device=dev)
    with pytest.raises(ValueError):
        ops.resize(x, (4, 4, 4), (1, 1, 1), out=x)
    with pytest.raises(ValueError):
        ops.resize(x.double(), (5, 5, 5), (1, 1, 1))
    with pytest.raises(RuntimeError, match='orders are 0, 1 or 3'):
        ops.resize(x, (5, 5, 5), (1, 2, 1))
    with pytest.raises(NotImplementedError):
        dp.resample_data_or_seg(x, (5, 5, 5), True, order=3)
    with pytest.raises(NotImplementedError):
        dp.resample_data_or_seg(x, (5, 5, 5), True, [0], 1, True, order_z=3)
    with pytest.raises(NotImplementedError):
        dp.resample_data_or_seg(x, (5, 5, 5), False, order=2)
    assert dp.resample_data_or_seg(x, (4, 4, 4), False) is x


# ---- B. the Python functions against the reference -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    z = np.load(G)
    assert list(z['geoms']) == GEOMS and list(z['names']) == CASES
    assert [tuple(o) for o in z['data_orders']] == DATA_ORDERS and [tuple(o) for o in z['seg_orders']] == SEG_ORDERS
    ip = {c: dict(zip(('mean', 'sd', 'percentile_00_5', 'percentile_99_5'), (float(v) for v in z['ip'][c]))) for c in (0, 1)}
    return z, ip, [int(c) for c in z['all_classes']]


def _geom(z, g):
    axis = int(z['geom/%s/axis' % g])
    return tuple(int(i) for i in z['geom/%s/new_shape' % g]), axis >= 0, ([axis] if axis >= 0 else None)


def _fragile(packed, shape):
    return np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize('g', GEOMS)
def test_resample_data_matches_the_reference(dev, golden, g):
    from multitalent_amd.preprocessing import device_preprocessing as dp
    z = golden[0]
    new_shape, sep, axis = _geom(z, g)
    data = torch.from_numpy(z['geom/%s/data' % g][:1]).to(dev)
    for order, order_z in DATA_ORDERS:
        out = dp.resample_data_or_seg(data, new_shape, False, axis, order, sep, order_z)
        ref = z['data/%s/%d%d' % (g, order, order_z)]
        assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
        d = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
        print('RESIZE-FIG resample_data_or_seg %s order (%d, %d) max |device - reference| %.3e (bound %.3e)' % (g, order, order_z, d, RAW_BOUND))
        if order == 0 and order_z == 0:
            assert d == 0.0
        assert d <= RAW_BOUND
    assert np.array_equal(data.cpu().numpy(), z['geom/%s/data' % g][:1])


@pytest.mark.parametrize('g', GEOMS)
def test_resample_seg_matches_the_reference_outside_fragile_voxels(dev, golden, g):
    from multitalent_amd.preprocessing import device_preprocessing as dp
    z = golden[0]
    new_shape, sep, axis = _geom(z, g)
    seg_np = z['geom/%s/seg' % g]
    for dtype in (torch.float32, torch.int16):
        seg = torch.from_numpy(seg_np.astype(np.float32)).to(dev).to(dtype)
        for order, order_z in SEG_ORDERS:
            out = dp.resample_data_or_seg(seg, new_shape, True, axis, order, sep, order_z)
            ref = z['seg/%s/%d%d' % (g, order, order_z)]
            keep = ~_fragile(z['fragile/%s/%d%d' % (g, order, order_z)], new_shape)
            got = out.cpu().numpy()
            assert out.dtype == dtype and got.shape == ref.shape
            print('RESIZE-FIG labels %s order (%d, %d) compared share %.4f mismatches outside fragile %d inside %d'
                  % (g, order, order_z, keep.mean(), int((got[0] != ref[0])[keep].sum()), int((got[0] != ref[0])[~keep].sum())))
            assert keep.mean() >= 0.90
            assert np.array_equal(got[0][keep], ref[0][keep])
            if order == 0:
                assert keep.all()


def test_resample_patient_decides_like_the_reference(dev, golden):
    from multitalent_amd.preprocessing import device_preprocessing as dp
    z = golden[0]
    for g, orders in (('up', dict(order_data=3, order_seg=1, order_z_data=3, order_z_seg=1)), ('iso_down', dict(order_data=1, order_seg=1)),
                      ('axis_last', dict(order_data=1, order_seg=0))):
        new_shape, sep, axis = _geom(z, g)
        sp = z['geom/%s/spacing' % g]
        data = torch.from_numpy(z['geom/%s/data' % g][:1]).to(dev)
        seg = torch.from_numpy(z['geom/%s/seg' % g].astype(np.float32)).to(dev)
        d, s = dp.resample_patient(data, seg, sp[:3], sp[3:], force_separate_z=None, **orders)
        od, oz = orders['order_data'], orders.get('order_z_data', 0)
        assert tuple(d.shape[1:]) == new_shape == tuple(s.shape[1:])
        assert torch.equal(d, dp.resample_data_or_seg(data, new_shape, False, axis, od, sep, oz))
        assert float(np.abs(d.cpu().numpy() - z['data/%s/%d%d' % (g, od, oz)]).max()) <= RAW_BOUND
        only_d, none = dp.resample_patient(data, None, sp[:3], sp[3:], force_separate_z=None, **orders)
        assert none is None and torch.equal(only_d, d)
    # force_separate_z=False (the signature's default) never separates
    new_shape, _, _ = _geom(z, 'up')
    sp = z['geom/up/spacing']
    data = torch.from_numpy(z['geom/up/data'][:1]).to(dev)
    d, _ = dp.resample_patient(data, None, sp[:3], sp[3:])
    assert torch.equal(d, dp.resample_data_or_seg(data, new_shape, False, None, 3, False, 0))


def _preprocessor(z, ip, name):
    from multitalent_amd.preprocessing import preprocessing as P
    schemes, masks = [str(s) for s in z[name + '/schemes']], [bool(m) for m in z[name + '/masks']]
    return getattr(P, str(z[name + '/class']))(dict(enumerate(schemes)), dict(enumerate(masks)), [0, 1, 2], ip), schemes, masks


@pytest.mark.parametrize('name', CASES)
def test_training_case_matches_the_reference(dev, golden, name):
    from multitalent_amd.preprocessing import device_preprocessing as dp
    z, ip, all_classes = golden
    pre, schemes, masks = _preprocessor(z, ip, name)
    g = str(z[name + '/geom'])
    sp = z['geom/%s/spacing' % g]
    props = {'original_spacing': sp[:3].copy(), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3, 4, 5]}
    data, seg = z['geom/%s/data' % g][:len(schemes)], z['geom/%s/seg' % g].astype(np.float32)
    all_data, out_props = pre.preprocess_training_case(data, seg, props, sp[3:], all_classes)
    assert all_data.is_cuda and all_data.dtype == torch.float32
    out, ref, ref_seg = all_data.cpu().numpy(), z[name + '/out'], z[name + '/out_seg'].astype(np.float32)
    assert out.shape == (ref.shape[0] + 1,) + ref.shape[1:]
    keep = ~_fragile(z[name + '/fragile'], ref.shape[1:])
    assert keep.mean() >= 0.90 and np.array_equal(out[-1][keep], ref_seg[keep])
    for c in range(len(ref)):
        bound = (RAW_BOUND if schemes[c] == 'noNorm' else CT_BOUND) + (0.0 if schemes[c] in ('CT', 'noNorm') else 2 * float(z[name + '/dev64']))
        d = np.abs(out[c] - ref[c])
        d64 = np.abs(out[c].astype(np.float64) - (ref[c].astype(np.float64) + z[name + '/d64'][c].astype(np.float64)))
        sel = keep if masks[c] else np.ones_like(keep)
        print('RESIZE-FIG %s channel %d (%s) max |device - reference| %.3e (float64-moment reference %.3e) bound %.3e'
              % (name, c, schemes[c], d[sel].max(), d64[sel].max(), bound))
        assert d[sel].max() <= bound, (c, d[sel].max(), bound)
    assert tuple(out_props['size_after_resampling']) == tuple(ref.shape[1:])
    assert np.array_equal(np.asarray(out_props['spacing_after_resampling']), sp[3:])
    assert out_props['valid_regions'] == [[1, 2], [3]] and out_props['valid_labels'] == [1, 2, 3, 4, 5]
    # class locations: the device's label map differs from the golden's on fragile voxels at most, so resolve them on the golden's
    locs = dp.class_locations(torch.from_numpy(np.ascontiguousarray(ref_seg)).to(dev), all_classes)
    assert list(locs.keys()) == all_classes
    for c in all_classes:
        want = z['%s/loc%d' % (name, c)]
        if len(want) == 0:
            assert isinstance(locs[c], list) and locs[c] == []
        else:
            assert isinstance(locs[c], np.ndarray) and locs[c].dtype == np.int64 and np.array_equal(locs[c], want)
    if not (out[-1] != ref_seg).any():
        for c in all_classes:
            assert np.array_equal(np.asarray(out_props['class_locations'][c]).reshape(-1, 3), z['%s/loc%d' % (name, c)])


def test_test_case_path_and_the_default_preprocessor(dev, golden):
    """resample_and_normalize of the new classes without keep_seg is the same full path; GenericPreprocessor keeps its own launches
    (its result differs from the order-(3, 3) class on a separately resampled case and equals resample_data / resample_seg)."""
    from multitalent_amd.preprocessing import device_preprocessing as dp
    from multitalent_amd.preprocessing import preprocessing as P
    z, ip, _ = golden
    sp = z['geom/up/spacing']
    data, seg = z['geom/up/data'][:1], z['geom/up/seg'].astype(np.float32)
    props = {'original_spacing': sp[:3].copy()}
    args = ({0: 'CT'}, {0: False}, [0, 1, 2], ip)
    d, s, p = P.Preprocessor3DDifferentResampling(*args).resample_and_normalize(data.copy(), sp[3:], dict(props), seg.copy())
    assert isinstance(d, np.ndarray) and isinstance(s, np.ndarray) and p['size_after_resampling'] == (13, 27, 25)
    ref = z['diff_up_ct/out']
    keep = ~_fragile(z['diff_up_ct/fragile'], ref.shape[1:])
    assert float(np.abs(d - ref).max()) <= CT_BOUND and np.array_equal(s[0][keep], z['diff_up_ct/out_seg'].astype(np.float32)[keep])
    d0, s0, _ = P.GenericPreprocessor(*args).resample_and_normalize(data.copy(), sp[3:], dict(props), seg.copy(), keep_seg=True)
    own = dp.resample_data(torch.from_numpy(data).to(dev), (13, 27, 25), [0], True)
    own = ((own.clamp(ip[0]['percentile_00_5'], ip[0]['percentile_99_5']) - ip[0]['mean']) / ip[0]['sd']).cpu().numpy()
    assert float(np.abs(d0 - own).max()) <= 1e-6 and float(np.abs(d0 - d).max()) > 1e-3
    assert np.array_equal(s0, dp.resample_seg(torch.from_numpy(seg).to(dev), (13, 27, 25), [0], True).cpu().numpy())


def test_run_writes_what_the_loader_reads(dev, golden, tmp_path):
    from multitalent_amd.training.dataloading.dataset_loading import load_dataset
    z, ip, all_classes = golden
    name = 'diff_mixed_ct2_mask'
    pre, schemes, _ = _preprocessor(z, ip, name)
    sp = z['geom/mixed/spacing']
    src, dst = tmp_path / 'cropped', tmp_path / 'out'
    src.mkdir()
    for case in ('a_000', 'a_001'):
        np.savez_compressed(src / (case + '.npz'), data=np.vstack((z['geom/mixed/data'][:1], z['geom/mixed/seg'].astype(np.float32))))
        with open(src / (case + '.pkl'), 'wb') as f:
            pickle.dump({'original_spacing': sp[:3].copy(), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3], 'note': case}, f)
    with open(src / 'dataset_properties.pkl', 'wb') as f:
        pickle.dump({'all_classes': all_classes}, f)
    pre.run([sp[3:]], str(src), str(dst), 'nnUNetData_plans_v2.3', num_threads=2)
    ref, ref_seg = z[name + '/out'], z[name + '/out_seg'].astype(np.float32)
    keep = ~_fragile(z[name + '/fragile'], ref.shape[1:])
    ds = load_dataset(str(dst / 'nnUNetData_plans_v2.3_stage0'))
    assert list(ds.keys()) == ['a_000', 'a_001']
    for case, entry in ds.items():
        arr = np.load(entry['data_file'])['data']
        assert arr.dtype == np.float32 and arr.shape == (2,) + ref.shape[1:]
        assert np.array_equal(arr[-1][keep], ref_seg[keep])
        assert float(np.abs(arr[0] - ref[0])[keep].max()) <= CT_BOUND + 2 * float(z[name + '/dev64'])
        p = entry['properties']
        assert p['note'] == case and tuple(p['size_after_resampling']) == tuple(ref.shape[1:])
        assert set(p['class_locations'].keys()) == set(all_classes) and len(p['class_locations'][7]) == 0
        for c in all_classes:
            for x, y, zz in np.asarray(p['class_locations'][c]).reshape(-1, 3)[:50]:
                assert arr[-1, x, y, zz] == c
    one = tmp_path / 'single'
    one.mkdir()
    pre._run_internal(sp[3:], 'a_000', str(one), str(src), None, all_classes)
    assert np.array_equal(np.load(one / 'a_000.npz')['data'], np.load(ds['a_000']['data_file'])['data'])


# ---- C. the chain at toy size --------------------------------------------------------------------------------------------------------
def test_v23_planner_through_the_driver_into_preprocess_patient(dev, tmp_path):
    from multitalent_amd.preprocessing import preprocessing as P
    from multitalent_amd.run.default_configuration import get_default_configuration
    e = PC.ToyEnvironment(tmp_path)
    try:
        e.plan_and_preprocess(PC.TASK901, '-pl3d', 'ExperimentPlanner3D_v23')
        task = PC.TASK901['name']
        out = os.path.join(e.preprocessed, task)
        plans = PC.load_pickle(os.path.join(out, 'nnUNetPlansv2.3_plans_3D.pkl'))
        assert plans['preprocessor_name'] == 'Preprocessor3DDifferentResampling' and plans['data_identifier'] == 'nnUNetData_plans_v2.3'
        stages = sorted(d for d in os.listdir(out) if d.startswith('nnUNetData_plans_v2.3_stage'))
        assert stages and len(plans['plans_per_stage']) == len(stages)
        last = len(stages) - 1
        target = plans['plans_per_stage'][last]['current_spacing']
        got = PC.load_cases(os.path.join(out, stages[-1]))
        assert len(got) == 5
        pre = P.Preprocessor3DDifferentResampling(plans['normalization_schemes'], plans['use_mask_for_norm'], plans['transpose_forward'],
                                                  plans['dataset_properties']['intensityproperties'])
        pre.run([target], os.path.join(e.cropped, task), str(tmp_path / 'by_hand'), 'by_hand', 2)
        PC.assert_same_cases(got, PC.load_cases(str(tmp_path / 'by_hand' / 'by_hand_stage0')))
        default = P.GenericPreprocessor(plans['normalization_schemes'], plans['use_mask_for_norm'], plans['transpose_forward'],
                                        plans['dataset_properties']['intensityproperties'])
        moved = 0
        for k, (a, props) in got.items():
            assert a.shape[1:] == PC.expected_shape(props, target, plans['transpose_forward'])
            assert np.array_equal(props['spacing_after_resampling'], target) and sorted(props['class_locations']) == [1, 2]
            moved += a.shape[1:] != tuple(props['size_after_cropping'][i] for i in plans['transpose_forward'])
        assert moved > 0                                                     # some case was actually resampled
        # a trainer built from those plans preprocesses an unseen file with the plans' class
        plans_file, output_folder, dataset_directory, batch_dice, stage, trainer_class = \
            get_default_configuration('3d_fullres', task, 'nnUNetTrainerV2', 'nnUNetPlansv2.3')
        tr = trainer_class(plans_file, 'all', output_folder=output_folder, dataset_directory=dataset_directory, batch_dice=batch_dice,
                           stage=stage, unpack_data=True, deterministic=False, fp16=False)
        tr.load_plans_file()
        tr.process_plans(tr.plans)
        image = os.path.join(e.raw, task, 'imagesTr', 'tiny_002_0000.nii.gz')          # 2.5 mm slices: resampled along the coarse axis
        d, s, props = tr.preprocess_patient([image])
        want, _, _ = pre.preprocess_test_case([image], target)
        assert isinstance(d, np.ndarray) and d.dtype == np.float32 and np.array_equal(d, want)
        stored = got['tiny_002'][0]
        assert d.shape == stored[:-1].shape and float(np.abs(d - stored[:-1]).max()) <= 1e-6
        other, _, _ = default.preprocess_test_case([image], target)
        assert other.shape == d.shape and float(np.abs(other - d).max()) > 1e-3        # order 0 along the coarse axis there
        tr.plans['preprocessor_name'] = 'Preprocessor3DBetterResampling'
        with pytest.raises(NotImplementedError, match='not on this path'):
            tr.preprocess_patient([image])
    finally:
        e.close()
