"""The references and the case census of tests/spatial_cases.py, on the CPU: every reference against scipy.ndimage (or an independent
statement of the same operation), every case shown to reach the branch it is named for, every exclusion cap on the reference alone,
and the host-side refusals of the data-augmentation classes.  No test here needs a GPU."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import spatial_cases as SC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'multitalent_amd', 'csrc')
IDS = lambda c: c.id
LATTICE = [c for c in SC.sample_cases() if c.kind == 'lattice']
GENERAL = [c for c in SC.sample_cases() if c.kind == 'general']


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_launch_constants_are_the_sources():
    prep, warp = _src('prep.hip'), _src('warp.hip')
    assert len(re.findall(r'blocks > %d\) blocks = %d;' % (SC.CAP_SAMPLE, SC.CAP_SAMPLE), prep + warp)) == 2       # affine, warp
    assert 'blocks > %d) blocks = %d;' % (SC.CAP_PYRAMID, SC.CAP_PYRAMID) in prep
    assert 'blocks > %d) blocks = %d;' % (SC.CAP_BLUR, SC.CAP_BLUR) in prep
    assert re.search(r'#define MT_BLUR_MAXR %d\b' % SC.BLUR_MAXR, prep)
    for name, val in (('MAXR', SC.ZB_MAXR), ('CHUNK', SC.ZB_CHUNK), ('TL', SC.ZB_TL), ('RB', SC.ZB_RB), ('TW', SC.ZB_TW), ('RW', SC.ZB_RW)):
        assert re.search(r'#define MT_ZB_%s %d\b' % (name, val), warp), name


# ================================================================================================================================
# A. the sampler
def _scipy_sample(c, d, n, ch, coords, order, vol=None, cval=None):
    """map_coordinates(mode='constant') of one channel; planar: slice by slice with the 2-D coordinates"""
    vol = d['src'][n, ch].astype(np.float64) if vol is None else vol
    cval = c.cval if cval is None else cval
    xd, xh, xw = coords
    if not c.planar:
        return ndimage.map_coordinates(vol, np.stack([xd, xh, xw]), order=order, mode='constant', cval=cval)
    return np.stack([ndimage.map_coordinates(vol[s], np.stack([xh[s], xw[s]]), order=order, mode='constant', cval=cval)
                     for s in range(vol.shape[0])])


def _scipy_labels(c, d, n, ch, coords, cval):
    """batchgenerators' interpolate_img(is_seg, order 1): ascending labels overwrite where their indicator reaches 0.5"""
    seg = d['src'][n, ch]
    out = np.zeros(c.out_shape)
    for lab in np.unique(seg):
        out[_scipy_sample(c, d, n, ch, coords, 1, (seg == lab).astype(np.float64), cval) >= 0.5] = lab
    return out


@pytest.mark.parametrize('case', LATTICE, ids=IDS)
def test_sampler_restatement_is_map_coordinates_on_the_lattice(case):
    """no exclusions: faces, .5 ties, mirrored taps, axes of length 1 and 2 — identical cval sets, values to 1e-13 of the range"""
    c, d = case, SC.sample_draw(case)
    ref, ins, coords = SC.sample_case_ref(c)
    worst = 0.0
    for n in range(c.N):
        for ch in range(c.C):
            if c.mode == 11:
                for cval in (c.cval, -1.0, 0.49):
                    assert np.array_equal(_scipy_labels(c, d, n, ch, coords[n], cval), ref[n, ch]), (n, ch, cval)
                continue
            sc = _scipy_sample(c, d, n, ch, coords[n], c.mode)
            assert np.array_equal(sc == c.cval, ~ins[n]) and np.array_equal(ref[n, ch] == c.cval, ~ins[n])
            if c.mode == 0:
                assert np.array_equal(sc, ref[n, ch])
            worst = max(worst, float(np.abs(sc - ref[n, ch]).max()))
    assert worst <= 1e-13 * np.ptp(d['src'])


@pytest.mark.parametrize('case', [c for c in LATTICE if c.entry == 'affine' and c.mode == 1], ids=IDS)
def test_lattice_cases_reach_faces_ties_and_the_outside(case):
    c, d = case, SC.sample_draw(case)
    assert int(np.prod(c.out_shape)) * c.N % SC.BLOCK != 0                       # a partial last block
    assert np.isin(d['mats'][:, :9], [0, 1, -1, 0.5, -0.5, 0.25, -0.25, 2]).all() and (d['mats'][:, 9:] * 4 % 1 == 0).all()
    xs = SC.sample_coords(c, d['mats'], None, None, 0)
    for x, n in list(zip(xs, c.in_shape))[1 if c.planar else 0:]:
        vals = set(np.unique(x).tolist())
        assert {-0.5, -0.25, 0.0, n - 1.0, n - 0.75, n - 0.5} <= vals and (n == 1 or 0.5 in vals)
    for n in range(c.N):                                      # every sample lies on the 1/8 lattice and has points inside and outside
        xs = SC.sample_coords(c, d['mats'], None, None, n)
        assert all((x * 8 % 1 == 0).all() for x in xs)
        ins = SC.inside_mask(c.in_shape, *xs)
        assert ins.any() and (~ins).any()


def test_lattice_mode1_sums_are_exact_in_float32():
    """why mode 1 may be compared bit for bit: every weight is a multiple of 2^-9 and the data are integers of magnitude <= 8"""
    for c in LATTICE:
        if c.mode == 1:
            d = SC.sample_draw(c)
            assert np.abs(d['src']).max() <= 8 and (d['src'] % 1 == 0).all()
            ref, _, _ = SC.sample_case_ref(c)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and (ref * 512 % 1 == 0).all()


def test_lattice_label_cases_hold_exact_ties():
    """mode 11: some output has two different labels at an indicator of exactly 0.5 — the larger one is expected"""
    for c in LATTICE:
        if c.mode == 11 and c.entry == 'affine' and not c.planar and c.in_shape == (4, 5, 6):
            d = SC.sample_draw(c)
            xs = SC.sample_coords(c, d['mats'], None, None, 0)
            seg = d['src'][0, 0]
            labs = np.unique(seg)
            ind = np.stack([SC.sample_ref((seg == l).astype(np.float64)[None], xs[0], xs[1], xs[2], 1, 0.0)[0][0] for l in labs])
            tie = (ind == 0.5).sum(0) == 2
            ref, _, _ = SC.sample_case_ref(c)
            assert tie.sum() > 20
            assert np.array_equal(ref[0, 0][tie], labs[np.where(ind == 0.5, np.arange(len(labs))[:, None, None, None], -1).max(0)][tie])


@pytest.mark.parametrize('case', GENERAL, ids=IDS)
def test_general_cases_exclude_at_most_one_percent(case):
    c, d = case, SC.sample_draw(case)
    ref, ins, coords = SC.sample_case_ref(c)
    ex = SC.general_exclusions(c, d, coords)
    print('SPATIAL-CENSUS %s excluded %d of %d, inside %d' % (c.id, ex.sum(), ex.size, ins.sum()))
    assert ex.mean() <= SC.EXCLUDE_CAP
    assert ins.mean() > 0.3 and (~ins).mean() > 0.02
    keep = ~ex
    worst = 0.0
    for n in range(c.N):                                      # and away from the exclusions the restatement is scipy's
        for ch in range(c.C):
            sc = _scipy_labels(c, d, n, ch, coords[n], c.cval) if c.mode == 11 else _scipy_sample(c, d, n, ch, coords[n], c.mode)
            worst = max(worst, float(np.abs(sc - ref[n, ch])[keep[n]].max()))
    assert worst <= (0.0 if c.mode in (0, 11) else 1e-12 * np.ptp(d['src'])), worst


@pytest.mark.parametrize('case', SC.stride_cases(), ids=IDS)
def test_stride_cases_pass_the_block_cap_with_data_on_both_sides(case):
    c, d = case, SC.sample_draw(case)
    total = c.N * int(np.prod(c.out_shape))
    first = SC.CAP_SAMPLE * SC.BLOCK
    assert total > first == 16777216
    od_split = first // (c.out_shape[1] * c.out_shape[2])
    xs = SC.sample_coords(c, d['mats'], d['field'], d['alpha'], 0, od_split - 2, od_split + 2)
    ins = SC.inside_mask(c.in_shape, *xs)
    assert ins[:2].any() and ins[2:].any()                     # inside the volume in the loop's first trip and in its second
    if c.entry == 'warp':
        assert d['field'].shape == (1, 2) + c.out_shape[1:] and float(d['alpha'][0]) == 4.0


# ================================================================================================================================
# B. the prefilter
def _prefilter_line(s):
    """the kernel's recursion on one line, in Python floats (double)"""
    z, n = -0.26794919243112270647, len(s)
    if n == 1:
        return list(s)
    zn = z ** (n - 1) if abs(z) ** (n - 1) > 0 else 0.0
    acc = 6.0 * (s[0] + zn * s[n - 1])
    z1, z2 = z, zn * zn / z
    for k in range(1, n - 1):
        acc += 6.0 * (z1 + z2) * s[k]
        z1 *= z
        z2 /= z
    c = [0.0] * n
    c[0] = acc / (1.0 - zn * zn)
    for k in range(1, n):
        c[k] = 6.0 * s[k] + z * c[k - 1]
    c[n - 1] = (z / (z * z - 1.0)) * (z * c[n - 2] + c[n - 1])
    for k in range(n - 2, -1, -1):
        c[k] = z * (c[k + 1] - c[k])
    return c


@pytest.mark.parametrize('n', [2, 3, 4, 21, 269, 280, 600])
def test_prefilter_recursion_is_spline_filter1d(n):
    """the two double recursions agree to 1e-13 of the line, also where pow(z, n - 1) squared leaves the normal range"""
    s = SC.rng('line', n).randn(n).astype(np.float32).astype(np.float64)
    ref = ndimage.spline_filter1d(s, 3, mode='mirror')
    got = np.array(_prefilter_line(list(s)))
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-13 * np.abs(s).max() * 6
    z = 0.26794919243112270647
    assert ((z ** (n - 1)) ** 2 < 2.3e-308) == (n >= 270)


def test_prefilter_cases_census():
    cases = SC.prefilter_cases()
    for bit in (1, 2, 4):
        assert sorted(c.shape[SC.PF_AXIS[bit]] for c in cases if c.axes == bit) == list(SC.PF_LENGTHS)
    assert sorted(set(c.axes for c in cases)) == [1, 2, 3, 4, 7]
    for c in cases:
        assert c.NC == 3
        for bit in (1, 2, 4):
            if c.axes & bit:
                lines = SC.prefilter_lines(c, bit)
                assert lines > SC.BLOCK and lines % SC.BLOCK != 0, (c.id, bit, lines)


def test_prefilter_reference_is_spline_filter():
    """all three passes against ndimage.spline_filter; the reference's float32 storage between passes costs a few ulp"""
    c = [k for k in SC.prefilter_cases() if k.axes == 7][0]
    x = SC.prefilter_draw(c)
    ref, linemax = SC.prefilter_ref(c, x)
    full = np.stack([ndimage.spline_filter(v.astype(np.float64), 3, mode='constant') for v in x])
    assert ref.dtype == np.float32 and np.abs(ref - full).max() < 1e-5 * np.abs(full).max()
    assert (linemax >= np.abs(ref).min()).all()
    one = [k for k in SC.prefilter_cases() if k.id == 'pf-a2-n1'][0]
    assert np.array_equal(SC.prefilter_ref(one, SC.prefilter_draw(one))[0], SC.prefilter_draw(one))         # length 1: untouched


# ================================================================================================================================
# C, D. the blurs
def test_blur_references_are_gaussian_filter():
    """one correlate1d pass per axis with gauss_weights = ndimage.gaussian_filter (reflect / constant), to 1e-13 of the data"""
    x = SC.rng('blurref').randn(2, 7, 19, 26)
    for sg in (0.3, 0.5, 1.0, 3.0, 8.0):
        for mode in ('reflect', 'constant'):
            cur = x.copy()
            for axis in range(3):
                c = SC.BlurCase('x', cur.shape[1:], axis, (sg, sg))
                cur = SC.blur_ref(c, cur, mode)
            full = np.stack([ndimage.gaussian_filter(v, float(np.float32(sg)), mode=mode, cval=0.0) for v in x])
            assert np.abs(cur - full).max() < 1e-13 * np.abs(x).max(), (sg, mode)


def test_reflect_blur_cases_census():
    cases = SC.reflect_blur_cases()
    assert sorted(set(SC.radius(s) for s in SC.RB_SIGMAS if s > 0)) == [0, 1, 2, 3, 4, 32] and SC.radius(8.0) == SC.BLUR_MAXR
    assert any(int(4.0 * float(np.float32(s))) != SC.radius(s) for s in SC.RB_SIGMAS if s > 0)          # the rounding of the radius matters
    assert any(s == 0 for s in SC.RB_SIGMAS) and any(s < 0 for s in SC.RB_SIGMAS)
    for axis in range(3):
        assert sorted(c.shape[axis] for c in cases if c.axis == axis and 'stride' not in c.id) == list(SC.RB_LENGTHS)
    assert any(SC.radius(s) > 2 * c.shape[c.axis] for c in cases for s in c.sigmas if s > 0)       # several reflections
    st = [c for c in cases if 'stride' in c.id][0]
    assert int(np.prod(st.shape)) > SC.CAP_BLUR * SC.BLOCK and st.axis == 0
    for s in SC.RB_REFUSED:                                    # the radius test of the kernel, in double on the float32 value
        assert not (np.float32(s) <= 0) and not (4.0 * float(np.float32(s)) + 0.5 < SC.BLUR_MAXR + 1)
    assert 4.0 * float(np.float32(8.124999)) + 0.5 < SC.BLUR_MAXR + 1


def test_zero_blur_cases_census():
    cases = SC.zero_blur_cases()
    assert sorted(set(SC.radius(s) for s in SC.ZB_SIGMAS if s > 0)) == [0, 1, 2, 3, 9, 64] and SC.radius(15.9) == SC.ZB_MAXR
    assert sum(SC.radius(s) < SC.ZB_RB for s in SC.ZB_SIGMAS if s > 0) == 4          # a thread's group of outputs wider than the radius
    for axis in (0, 1):
        for inner in (1, 65):
            got = sorted(c.shape[axis] for c in cases if c.axis == axis and c.id.endswith('-in%d' % inner))
            assert got == list(SC.ZB_LENGTHS)
            for c in cases:
                if c.axis == axis and c.id.endswith('-in%d' % inner):
                    assert (c.shape[1] * c.shape[2] if axis == 0 else c.shape[2]) == inner
    assert sorted(set(SC.zero_blur_tiles(c)[0] for c in cases if c.axis < 2)) == [1, 2, 3]      # tiles along the axis (64 outputs each)
    assert sorted(set(SC.zero_blur_tiles(c)[1] for c in cases if c.axis < 2)) == [1, 2]         # tiles across it (64 lanes each)
    assert any(c.shape[c.axis] % SC.ZB_RB for c in cases if c.axis < 2) and any(c.shape[c.axis] % SC.ZB_TL == 1 for c in cases if c.axis < 2)
    w = [c for c in cases if c.axis == 2 and 'rows' in c.id]
    assert sorted(set(c.shape[2] for c in w)) == list(SC.ZB_WIDTHS)
    assert sorted(set(SC.zero_blur_tiles(c)[0] for c in w)) == [1, 2] and sorted(set(SC.zero_blur_tiles(c)[1] for c in w)) == [1, 2]
    assert all(c.shape[0] * c.shape[1] % SC.ZB_RW for c in w)                                   # D*H is no multiple of 8: a partial row tile
    assert any(SC.radius(s) > c.shape[c.axis] for c in cases for s in c.sigmas if s > 0)        # r > L
    many = [c for c in cases if len(c.sigmas) > SC.ZB_CHUNK]
    assert sorted(set((c.axis, len(c.sigmas)) for c in many)) == [(a, n) for a in range(3) for n in (33, 70)]
    for c in many:
        assert c.shape == (3, 5, 7)
        pos = [s for s in c.sigmas if s > 0]
        assert len(set(pos)) == len(pos) and all(SC.radius(s) <= SC.ZB_MAXR for s in pos)
        for c0 in range(0, len(c.sigmas), SC.ZB_CHUNK):
            chunk = c.sigmas[c0:c0 + SC.ZB_CHUNK]
            assert (0.0 in chunk and min(chunk) < 0) or len(chunk) < 12
    assert {c.data for c in cases} == {'randn', 'impulse', 'ramp'}
    c = [k for k in cases if k.data == 'impulse'][0]
    x = SC.blur_draw(c)
    assert x[0, 0, 0, 0] == 1 and x[0, -1, -1, -1] == -2 and np.count_nonzero(x[0]) == 2


# ================================================================================================================================
# E. the label pyramid
def test_pyramid_index_is_scipy_zoom_for_every_pair_below_200():
    bad = 0
    for n_in in range(1, 200):
        src = np.arange(n_in, dtype=np.float64)
        for n_out in range(1, 200):
            z = ndimage.zoom(src, n_out / n_in, order=0, mode='nearest', grid_mode=True)
            bad += z.shape != (n_out,) or not np.array_equal(z, SC.pyramid_index(n_in, n_out))
    assert bad == 0


def test_pyramid_cases_census():
    cases = SC.pyramid_cases()
    for axis in range(3):
        assert sorted((c.in_shape[axis], c.out_shape[axis]) for c in cases if 'stride' not in c.id) == sorted(SC.PY_PAIRS)
    assert [c.kind for c in cases].count('image') == 1
    for c in cases:
        x = SC.pyramid_draw(c)
        assert (x == -1.0).any()
        if c.kind == 'image':
            assert (x % 1 != 0).any()
        if 'stride' not in c.id:                               # the reference is the per-axis index rule
            i = [SC.pyramid_index(a, b) for a, b in zip(c.in_shape, c.out_shape)]
            assert np.array_equal(SC.pyramid_ref(c, x, False), x[:, i[0][:, None, None], i[1][None, :, None], i[2][None, None, :]])
            assert not (SC.pyramid_ref(c, x, True) == -1.0).any()
    st = [c for c in cases if 'stride' in c.id][0]
    assert st.NC * int(np.prod(st.out_shape)) > SC.CAP_PYRAMID * SC.BLOCK


# ================================================================================================================================
# the refusals that need no device
@pytest.mark.parametrize('cval', [0.5, 1, 3.0, float('inf')])
def test_label_rule_refuses_a_cval_the_reference_would_turn_into_the_largest_label(cval):
    from multitalent_amd.training.data_augmentation.spatial import SpatialTransformDevice, affine_sample, warp_sample
    with pytest.raises(NotImplementedError, match='largest label'):
        SpatialTransformDevice((8, 8, 8), border_cval_seg=cval)
    with pytest.raises(NotImplementedError, match='largest label'):
        affine_sample(None, None, (1, 1, 1), 1, cval=cval, is_seg=True)
    with pytest.raises(NotImplementedError, match='largest label'):
        warp_sample(None, None, (1, 1, 1), 1, None, None, cval=cval, is_seg=True)


def test_label_rule_accepts_what_the_kernel_implements():
    from multitalent_amd.training.data_augmentation.spatial import SpatialTransformDevice
    for cval in (-1, 0, 0.49):
        assert SpatialTransformDevice((8, 8, 8), border_cval_seg=cval).cval_seg == cval
    assert SpatialTransformDevice((8, 8, 8), border_cval_seg=2, order_seg=0).cval_seg == 2        # order 0 is plain nearest sampling


def test_reference_label_rule_gives_the_largest_label_outside_for_cval_half():
    """what the message says the reference does, on scipy"""
    seg = np.array([[1., 2.], [0., 3.]])
    out = np.zeros(3)
    co = np.array([[-1.0, 0.0, 5.0], [0.0, 0.0, 0.0]])
    for lab in np.unique(seg):
        out[ndimage.map_coordinates((seg == lab).astype(float), co, order=1, mode='constant', cval=0.5) >= 0.5] = lab
    assert out.tolist() == [3.0, 1.0, 3.0]


@pytest.mark.parametrize('sigma', [(0.5, 8.125), (0.5, 9.0), (13.0, 13.0), (0.5, float('nan')), (float('nan'), 1.0)])
def test_gaussian_blur_transform_refuses_a_radius_above_32(sigma):
    from multitalent_amd.training.data_augmentation.color import GaussianBlurDevice, check_blur_sigma
    with pytest.raises(ValueError, match='radius above 32'):
        GaussianBlurDevice(blur_sigma=sigma)
    with pytest.raises(ValueError, match='radius above 32'):
        check_blur_sigma(np.array([[0.0, sigma[1]], [sigma[0], -1.0]]), 'x')


def test_gaussian_blur_transform_accepts_every_radius_up_to_32():
    from multitalent_amd.training.data_augmentation.color import GaussianBlurDevice, check_blur_sigma
    assert GaussianBlurDevice(blur_sigma=(0.5, 8.0)).sigma == (0.5, 8.0)
    assert GaussianBlurDevice().sigma == (0.5, 1.)
    assert check_blur_sigma([0.0, -3.0, 8.124999, float('-inf')], 'x').dtype == np.float32
