"""Elastic deformation of the device SpatialTransform and the MaskTransform of the chain, against scipy.ndimage — the library
batchgenerators' elastic_deform_coordinates and interpolate_img compute with: the zero-padded Gaussian vs gaussian_filter(mode=
'constant'), the warped sampler vs map_coordinates over M (g + alpha f) + centre with the SAME float32 field on both sides, the
per-label segmentation rule under a field, the planar (dummy 2D) mode, and the transform / the chain built on them."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu


def _cases(rs, n, in_shape):
    """tests/test_spatial_gpu.py's matrices: identity, a rotation, rotations with anisotropic scaling, then off-centre crops."""
    from multitalent_amd.training.data_augmentation.spatial import rotation_matrix_3d
    mats = np.zeros((n, 12), np.float32)
    for i in range(n):
        m = rotation_matrix_3d(*rs.uniform(-0.6, 0.6, 3)) if i else np.eye(3)
        m = rs.uniform(0.7, 1.4, 3)[:, None] * m if i > 1 else m
        ctr = np.array(in_shape) / 2. - 0.5 + (rs.uniform(-4, 4, 3) if i > 2 else 0)
        mats[i, :9], mats[i, 9:] = m.reshape(-1), ctr
    return mats


def _to(dev, a):
    """a device copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a)).to(dev)


def _warped_coords(m, ctr, out_shape, alpha, field):
    """M (g + alpha f) + centre in float64; field [ndim, *out_shape]."""
    g = np.stack(np.meshgrid(*[np.arange(s) - (s - 1) / 2. for s in out_shape], indexing='ij')).astype(np.float64)
    g = g + float(alpha) * field.astype(np.float64)
    nd = len(out_shape)
    return (m @ g.reshape(nd, -1) + ctr[:, None]).reshape((nd,) + tuple(out_shape))


IN_SHAPE, OUT_SHAPE, N, C = (20, 26, 30), (12, 16, 18), 5, 2
ALPHA = np.array([0, 900, 400, 60, 150], np.float32)
SIGMA = [None, 9, 13, 3, 5]


@functools.lru_cache(maxsize=None)
def _warp_case():
    """data, matrices, float32 fields (scipy's zero-padded Gaussian of uniform noise) and the float64 reference coordinates, shared
    by the sampler tests and never modified."""
    rs = np.random.RandomState(11)
    x = rs.randn(N, C, *IN_SHAPE).astype(np.float32)
    mats = _cases(rs, N, IN_SHAPE)
    field = np.zeros((N, 3) + OUT_SHAPE, np.float32)
    for n in range(1, N):
        for d in range(3):
            field[n, d] = ndimage.gaussian_filter(rs.random_sample(OUT_SHAPE) * 2 - 1, SIGMA[n], mode='constant', cval=0).astype(np.float32)
    co = [_warped_coords(mats[n, :9].reshape(3, 3).astype(np.float64), mats[n, 9:].astype(np.float64), OUT_SHAPE, ALPHA[n], field[n])
          for n in range(N)]
    for a in (x, mats, field):
        a.setflags(write=False)
    return x, mats, field, co


def _blur_case(dev, shape, sigma):
    from multitalent_amd.training.data_augmentation.spatial import gaussian_filter_zero_device
    rs = np.random.RandomState(0)
    x = (2 * rs.random_sample(shape) - 1).astype(np.float32)
    sg = np.broadcast_to(np.asarray(sigma, np.float32), shape[:2])
    t = torch.from_numpy(x).to(dev)
    got = gaussian_filter_zero_device(t, sg).cpu().numpy()
    assert np.array_equal(t.cpu().numpy(), x)                         # the input is not modified
    return x, sg, got


@pytest.mark.parametrize("shape,sigma", [((1, 4, 7, 19, 26), [[9, 13, 2.3, 15.8]]),        # r = 36, 52, 9, 63
                                         ((2, 1, 1, 19, 26), [[9], [13]]),                  # the 2-D field of the planar mode
                                         ((1, 1, 2, 70, 300), 9), ((1, 1, 70, 3, 300), 9)])  # several tiles along W and along H / D
def test_zero_padded_blur_matches_scipy(dev, shape, sigma):
    """2e-6 (the project's blur tolerance) of the OUTPUT's range: zero padding with sigma >= 9 shrinks the output to about 1/500
    of the input, so a bound on the input's range would be vacuous.  Three float32-rounded passes sit at <= 4e-7 of it."""
    x, sg, got = _blur_case(dev, shape, sigma)
    for n in range(shape[0]):
        for c in range(shape[1]):
            a = x[n, c].astype(np.float64)
            a = a[0] if a.shape[0] == 1 else a                        # an axis of length 1 is skipped: scipy's 2-D filter
            ref = ndimage.gaussian_filter(a, float(sg[n, c]), mode='constant', cval=0).reshape(shape[2:])
            err = np.abs(got[n, c] - ref).max()
            print(shape, float(sg[n, c]), 'max err / max |ref| = %.3g' % (err / np.abs(ref).max()))
            assert err < 2e-6 * np.abs(ref).max(), (n, c, err, np.abs(ref).max())


def test_zero_padded_blur_copies_and_refuses(dev):
    from multitalent_amd import _lib
    from multitalent_amd.training.data_augmentation.spatial import gaussian_filter_zero_device
    x, sg, got = _blur_case(dev, (1, 3, 7, 19, 26), [[0, 9, 0]])
    assert np.array_equal(got[0, 0], x[0, 0]) and np.array_equal(got[0, 2], x[0, 2])        # sigma 0: bit-identical copies
    assert not np.array_equal(got[0, 1], x[0, 1])
    t = torch.from_numpy(x).to(dev)
    with pytest.raises(ValueError):
        gaussian_filter_zero_device(t, [[9, 16.2, 0]])
    # the library itself refuses before any launch: the destination keeps its contents, also for the channel with a valid sigma
    dst = torch.full_like(t, 77.0)
    sig = np.array([9, 16.2, 0], np.float32)
    rc = _lib.load().mt_gaussian_blur_axis_zero(t.data_ptr(), dst.data_ptr(), 3, 7, 19, 26, 2, sig.ctypes.data_as(_lib.c_float_p),
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b'sigma[1]' in _lib.load().mt_last_error()
    assert bool((dst == 77.0).all())


@pytest.mark.parametrize("order", [3, 1, 0])
def test_warp_sample_matches_map_coordinates(dev, order):
    """Only the sampler is under test: the same float32 field goes to the kernel and, as float64, into the reference coordinates.
    Orders 3 and 1: the affine test's bound 2e-5 * 8 away from outputs whose coordinate is within 1e-4 of a volume face; order 0:
    exact away from coordinates within 1e-4 of a .5 rounding tie.  At most 1 % of the outputs may be excluded."""
    from multitalent_amd.training.data_augmentation.spatial import warp_sample
    x, mats, field, coords = _warp_case()
    got = warp_sample(_to(dev, x), mats, OUT_SHAPE, order, _to(dev, field), ALPHA, cval=-3.0).cpu().numpy()
    excluded = 0
    for n in range(N):
        co = coords[n]
        skip = np.zeros(OUT_SHAPE, bool)
        for d in range(3):
            if order == 0:
                skip |= np.abs(co[d] + 0.5 - np.round(co[d] + 0.5)) < 1e-4
            else:
                skip |= (np.abs(co[d]) < 1e-4) | (np.abs(co[d] - (IN_SHAPE[d] - 1)) < 1e-4)
        excluded += skip.sum()
        for c in range(C):
            ref = ndimage.map_coordinates(x[n, c].astype(np.float64), co, order=order, mode='constant', cval=-3.0)
            err = np.abs(got[n, c] - ref)[~skip].max()
            print('order', order, 'sample', n, 'channel', c, 'max err %.3g' % err, 'excluded', int(skip.sum()))
            if order == 0:
                assert err == 0, (n, c, err)
            else:
                assert err < 2e-5 * 8, (order, n, c, err)
    assert excluded <= 0.01 * N * np.prod(OUT_SHAPE)
    assert (got == -3.0).any() and (got != -3.0).any()              # coordinates inside and outside the volume both occur


def test_warp_sample_with_alpha_zero_is_affine_sample(dev):
    """alpha == 0: the field is not read (it is NaN here) and the result is mt_affine_sample's bit for bit, in all four modes and in
    the planar mode."""
    from multitalent_amd.training.data_augmentation.spatial import affine_sample, warp_sample
    x, mats, _, _ = _warp_case()
    t = _to(dev, x)
    lab = torch.from_numpy(np.random.RandomState(4).randint(-1, 4, size=x.shape).astype(np.float32)).to(dev)
    nan3 = torch.full((N, 3) + OUT_SHAPE, float('nan'), device=dev)
    zero = np.zeros(N, np.float32)
    for src, order, is_seg in ((t, 0, False), (t, 1, False), (t, 3, False), (lab, 1, True)):
        a = affine_sample(src, mats, OUT_SHAPE, order, cval=-3.0, is_seg=is_seg)
        w = warp_sample(src, mats, OUT_SHAPE, order, nan3, zero, cval=-3.0, is_seg=is_seg)
        assert torch.equal(a, w), (order, is_seg)
    pm = np.array(mats)
    pm[:, 9] = 0
    out = (IN_SHAPE[0],) + OUT_SHAPE[1:]
    nan2 = torch.full((N, 2) + OUT_SHAPE[1:], float('nan'), device=dev)
    for order in (1, 3):
        a = affine_sample(t, pm, out, order, cval=-3.0, planar=True)
        w = warp_sample(t, pm, out, order, nan2, zero, cval=-3.0, planar=True)
        assert torch.equal(a, w), order


def test_segmentation_rule_under_a_field(dev):
    """interpolate_img(seg, coords, order=1, 'constant', cval, is_seg=True) restated with map_coordinates, over the displaced
    coordinates: exact away from interpolated indicators within 1e-4 of 0.5, which may be at most 1 % of the outputs."""
    from multitalent_amd.training.data_augmentation.spatial import warp_sample
    _, mats, field, coords = _warp_case()
    rs = np.random.RandomState(2)
    coarse = rs.randint(-1, 4, size=(N, 1, 5, 7, 8)).astype(np.float32)
    seg = np.ascontiguousarray(np.kron(coarse, np.ones((1, 1, 4, 4, 4), np.float32))[:, :, :IN_SHAPE[0], :IN_SHAPE[1], :IN_SHAPE[2]])
    got = warp_sample(_to(dev, seg), mats, OUT_SHAPE, 1, _to(dev, field), ALPHA, cval=-1.0,
                      is_seg=True).cpu().numpy()
    bad = fragile_total = 0
    for n in range(N):
        ref = np.zeros(OUT_SHAPE, np.float32)
        fragile = np.zeros(OUT_SHAPE, bool)
        for c in np.unique(seg[n, 0]):
            r = ndimage.map_coordinates((seg[n, 0] == c).astype(float), coords[n], order=1, mode='constant', cval=-1.0)
            ref[r >= 0.5] = c
            fragile |= np.abs(r - 0.5) < 1e-4
        bad += (got[n, 0][~fragile] != ref[~fragile]).sum()
        fragile_total += fragile.sum()
    print('segmentation rule: mismatches', int(bad), 'excluded', int(fragile_total))
    assert bad == 0 and fragile_total <= 0.01 * N * np.prod(OUT_SHAPE)
    assert len(np.unique(got)) == 5


@pytest.mark.parametrize("order", [3, 1])
def test_planar_warp_matches_2d_map_coordinates(dev, order):
    """dummy 2D: one 2-component field over (H, W) shared by all slices, the slice axis untouched; per-slice 2-D map_coordinates,
    the planar affine test's bound 1e-4."""
    from multitalent_amd.training.data_augmentation.spatial import warp_sample
    rs = np.random.RandomState(5)
    D, in_hw, out_hw, n_s = 6, (26, 30), (16, 18), 3
    x = rs.randn(n_s, 1, D, *in_hw).astype(np.float32)
    mats = np.zeros((n_s, 12), np.float32)
    for n in range(n_s):
        a = rs.uniform(-0.5, 0.5) if n else 0.0
        r2 = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).T * (rs.uniform(0.7, 1.4) if n > 1 else 1.0)
        m = np.eye(3); m[1:, 1:] = r2
        mats[n, :9] = m.reshape(-1); mats[n, 9:] = [0, in_hw[0] / 2. - 0.5, in_hw[1] / 2. - 0.5]
    field = np.stack([[ndimage.gaussian_filter(rs.random_sample(out_hw) * 2 - 1, 3, mode='constant').astype(np.float32) for _ in range(2)]
                      for _ in range(n_s)])
    alpha = np.array([2.0 / np.abs(field[n]).max() for n in range(n_s)], np.float32)          # displacements of up to 2 voxels
    got = warp_sample(torch.from_numpy(x).to(dev), mats, (D,) + out_hw, order, torch.from_numpy(field).to(dev), alpha, cval=0.0,
                      planar=True).cpu().numpy()
    for n in range(n_s):
        co = _warped_coords(mats[n, :9].reshape(3, 3)[1:, 1:].astype(np.float64), mats[n, 10:].astype(np.float64), out_hw, alpha[n], field[n])
        edge = np.zeros(out_hw, bool)
        for k in range(2):
            edge |= (np.abs(co[k]) < 1e-4) | (np.abs(co[k] - (in_hw[k] - 1)) < 1e-4)
        for d in range(D):
            ref = ndimage.map_coordinates(x[n, 0, d].astype(np.float64), co, order=order, mode='constant', cval=0.0)
            assert np.abs(got[n, 0, d] - ref)[~edge].max() < 1e-4, (n, d)


@pytest.mark.parametrize("dummy_2d", [False, True])
def test_transform_is_warp_sample_of_its_own_draws(dev, dummy_2d):
    """The transform's outputs are warp_sample of the same inputs with the field rebuilt from last_elastic (seed -> noise ->
    gaussian_filter_zero_device) and the drawn matrices, bit for bit, and they differ from the undeformed sampling."""
    from multitalent_amd.training.data_augmentation.spatial import (SpatialTransformDevice, affine_sample, elastic_noise,
                                                                    gaussian_filter_zero_device, warp_sample)
    rs = np.random.RandomState(3)
    in_shape = (12, 30, 30) if dummy_2d else (20, 30, 30)
    x = torch.from_numpy(rs.randn(2, 1, *in_shape).astype(np.float32)).to(dev)
    s = torch.from_numpy(rs.randint(0, 3, size=(2, 1) + in_shape).astype(np.float32)).to(dev)
    patch = (12, 20, 20)
    kw = dict(p_el_per_sample=1, alpha=(300, 300), sigma=(3, 5), border_cval_seg=-1, dummy_2d=dummy_2d)
    np.random.seed(0)
    st = SpatialTransformDevice(patch, do_elastic_deform=True, **kw)
    d, g = st(x, s)
    assert d.shape == (2, 1) + patch and g.shape == (2, 1) + patch and bool(torch.isfinite(d).all())
    assert set(np.unique(g.cpu().numpy())) <= {-1.0, 0.0, 1.0, 2.0}
    assert all(e is not None and e[0] == 300 and 3 <= e[1] <= 5 for e in st.last_elastic)
    nd, fshape = (2, (1,) + patch[1:]) if dummy_2d else (3, patch)
    field = torch.stack([gaussian_filter_zero_device(elastic_noise(seed, nd, fshape, dev), np.full((nd, 1), sg, np.float32))
                         for _, sg, seed in st.last_elastic])
    field = field.reshape((2, nd) + (patch[1:] if dummy_2d else patch)).contiguous()
    alpha = np.array([e[0] for e in st.last_elastic], np.float32)
    assert float(field.abs().max()) * 300 > 0.5                       # the deformation moves voxels by a visible amount
    d_ref = warp_sample(x, st.last_mats, patch, 3, field, alpha, 0, planar=dummy_2d)
    g_ref = warp_sample(s, st.last_mats, patch, 1, field, alpha, -1, is_seg=True, planar=dummy_2d)
    assert torch.equal(d, d_ref) and torch.equal(g, g_ref)
    assert not torch.equal(d, affine_sample(x, st.last_mats, patch, 3, 0, planar=dummy_2d))
    np.random.seed(0)
    d0, _ = SpatialTransformDevice(patch, do_elastic_deform=False, **kw)(x, s)
    assert d0.shape == d.shape and not torch.equal(d, d0)


def test_chain_with_elastic_and_mask(dev):
    """MoreDADeviceAugmenter with elastic deformation on every sample and use_mask_for_norm for channel 0: the channel is 0
    wherever the augmented target is negative, and the target still carries its -1 (the trainers remove it later)."""
    from multitalent_amd.training.data_augmentation.color import MoreDADeviceAugmenter, default_3d_augmentation_params
    from multitalent_amd.training.data_augmentation.spatial import get_patch_size
    params = default_3d_augmentation_params()
    params.update(do_elastic=True, p_eldef=1.0, mask_was_used_for_normalization={0: True})
    assert params['elastic_deform_alpha'] == (0., 900.) and params['elastic_deform_sigma'] == (9., 13.)
    ps = (12, 24, 24)
    bps = tuple(int(i) for i in get_patch_size(ps, params['rotation_x'], params['rotation_y'], params['rotation_z'], (0.85, 1.25)))
    rs = np.random.RandomState(6)

    def batch():
        data = (rs.randn(2, 1, *bps) + 3).astype(np.float32)
        seg = rs.randint(0, 3, size=(2, 1) + bps).astype(np.float32)
        seg[:, :, :, :bps[1] // 2 - 3] = -1                          # outside the non-zero mask
        return {'data': data, 'seg': seg, 'properties': [None, None], 'keys': ['a', 'b']}

    np.random.seed(1)
    torch.manual_seed(1)
    aug = MoreDADeviceAugmenter(iter([batch(), batch()]), ps, params, dev)
    n = 0
    for out in aug:
        data, target = out['data'], out['target']
        assert tuple(data.shape) == (2, 1) + ps and tuple(target.shape) == (2, 1) + ps
        assert bool(torch.isfinite(data).all()) and bool(torch.isfinite(target).all())
        assert all(e is not None for e in aug.spatial.last_elastic)
        outside = target[:, 0] < 0
        assert bool(outside.any()) and bool((target == -1).any())
        assert bool((data[:, 0][outside] == 0).all()) and bool((data[:, 0][~outside] != 0).any())
        n += 1
    assert n == 2
