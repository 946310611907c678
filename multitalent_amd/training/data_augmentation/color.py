"""Intensity augmentations of nnU-Net's moreDA chain on the device (data_augmentation_moreDA.py:86-106): GaussianNoise,
GaussianBlur, BrightnessMultiplicative, ContrastAugmentation, SimulateLowResolution and the two GammaTransforms.  Only the noise
is torch glue (`torch.randn_like`, asynchronous).  BrightnessMultiplicative, ContrastAugmentation and the GammaTransforms run on
`mt_channel_stats` (min, max, mean, sd per channel in one pass, kept in device memory) and `mt_intensity_apply` (one fused
in-place pass for the whole batch, the drawn parameters in the kernel arguments): all numpy draws of a batch are made first
(`plan`), then one launch group per transform is issued, and nothing is read back from the device — measured with every
probability 1 at B = 2, 48x192x192: the four together 0.22 ms per batch with one channel, 0.36 ms with four (the loops of torch
operations with `float()` reads they replace: 1.05 / 4.09 ms with the host blocked throughout), pinned against the
float64 evaluation of those loops in tests/test_intensity_gpu.py.  The two filtering / resampling transforms run on
HIP kernels: GaussianBlur on `mt_gaussian_blur_axis` (= scipy.ndimage.gaussian_filter), SimulateLowResolution on
`mt_downsample_seg_nearest` (order-0 resize) followed by `mt_spline_prefilter3` + `mt_affine_sample` (order-3 resize), each pinned
against its scipy formulation in tests/test_spatial_gpu.py.  The RANDOM-PARAMETER logic (which samples / channels, sigma and zoom
draws) restates batchgenerators' augment_* functions (third party, absent in the build container, batchgenerators>=0.23) from
the published source: parity UNPINNED."""
import numpy as np
import torch

from ... import _lib


def _range_pick(lo, hi):
    """batchgenerators' two-sided draw: below 1 with probability 1/2 when the range allows it."""
    if np.random.random() < 0.5 and lo < 1:
        return np.random.uniform(lo, 1)
    return np.random.uniform(max(lo, 1), hi)


class GaussianNoiseDevice:
    def __init__(self, noise_variance=(0, 0.1), p_per_sample=0.1):
        self.var, self.p = noise_variance, p_per_sample

    def __call__(self, data):
        for b in range(data.shape[0]):
            if np.random.uniform() < self.p:
                v = self.var[0] if self.var[0] == self.var[1] else np.random.uniform(self.var[0], self.var[1])
                data[b] += torch.randn_like(data[b]) * v          # augment_gaussian_noise passes the "variance" as the std
        return data


BLUR_MAX_RADIUS = 32          # mt_gaussian_blur_axis never clamps the radius int(4 sigma + 0.5): a larger one gives a NaN channel


def check_blur_sigma(sigma, who):
    """ValueError for a sigma mt_gaussian_blur_axis cannot filter with: a radius above BLUR_MAX_RADIUS (sigma >= 8.125) or a NaN.
    The comparison is the kernel's, in double on the float32 value; -> the sigmas as a float32 array."""
    sg = np.asarray(sigma, dtype=np.float32)
    ok = (sg <= 0) | (4.0 * sg.astype(np.float64) + 0.5 < BLUR_MAX_RADIUS + 1)          # false for a NaN as well
    if not ok.all():
        raise ValueError("%s: sigma %s needs a radius above %d (or is NaN); the device filter never clamps a radius"
                         % (who, sg[~ok], BLUR_MAX_RADIUS))
    return sg


def gaussian_filter_device(x, sigma):
    """scipy.ndimage.gaussian_filter(x[n, c], sigma[n, c], order=0) (mode 'reflect', truncate 4) for every (sample, channel) of a
    [N, C, D, H, W] device tensor; sigma <= 0 leaves that channel untouched.  Axis order D, H, W like scipy; every pass rounds to
    float32 like scipy does for float32 input.  A sigma whose radius int(4 sigma + 0.5) exceeds 32, or a NaN, is a ValueError."""
    assert x.is_cuda and x.dim() == 5 and x.dtype == torch.float32
    N, C, D, H, W = (int(i) for i in x.shape)
    sg = torch.as_tensor(check_blur_sigma(sigma, 'gaussian_filter_device').reshape(N * C)).to(x.device)
    lib = _lib.load()
    st = torch.cuda.current_stream(x.device).cuda_stream
    src = x.contiguous()
    t0, t1 = torch.empty_like(src), torch.empty_like(src)          # D: src -> t0, H: t0 -> t1, W: t1 -> t0 (the input is never written)
    for axis, (a, b) in enumerate(((src, t0), (t0, t1), (t1, t0))):
        _lib.check(lib.mt_gaussian_blur_axis(a.data_ptr(), b.data_ptr(), N * C, D, H, W, axis, sg.data_ptr(), st), 'gaussian_blur_axis')
    a = t0
    return a


class GaussianBlurDevice:
    """GaussianBlurTransform((0.5, 1.), different_sigma_per_channel=True, p_per_sample=0.2, p_per_channel=0.5)
    (data_augmentation_moreDA.py:87-88; batchgenerators augment_gaussian_blur): per chosen sample, every channel is blurred with
    probability p_per_channel with its own sigma ~ U(blur_sigma)."""

    def __init__(self, blur_sigma=(0.5, 1.), different_sigma_per_channel=True, p_per_channel=0.5, p_per_sample=0.2):
        check_blur_sigma(blur_sigma, 'GaussianBlurDevice(blur_sigma)')
        self.sigma, self.per_channel, self.ppc, self.p = blur_sigma, different_sigma_per_channel, p_per_channel, p_per_sample

    def _draw(self):
        return self.sigma[0] if self.sigma[0] == self.sigma[1] else np.random.uniform(self.sigma[0], self.sigma[1])

    def __call__(self, data):
        N, C = int(data.shape[0]), int(data.shape[1])
        sg = np.zeros((N, C), dtype=np.float32)
        for b in range(N):
            if np.random.uniform() < self.p:
                shared = None if self.per_channel else self._draw()
                for c in range(C):
                    if np.random.uniform() <= self.ppc:
                        sg[b, c] = self._draw() if self.per_channel else shared
        if not (sg > 0).any():
            return data
        return gaussian_filter_device(data, sg)


def simulate_low_resolution_device(x, target_shape, planar=False):
    """resize(resize(x, target_shape, order=0), x.shape, order=3) with skimage's mode='edge', anti_aliasing=False for ONE channel
    volume x [D, H, W] (augment_linear_downsampling_scipy's body): nearest sampling at floor((o + 0.5) in/out), then the cubic
    B-spline resize at (o + 0.5) in/out - 0.5 behind 12 voxels of edge padding.  planar: axis 0 keeps its size (ignore_axes=(0,)),
    every slice is resized on its own."""
    from ... import ops
    from ...preprocessing.device_preprocessing import _zoom3
    shp = tuple(int(i) for i in x.shape)
    tgt = tuple(int(i) for i in target_shape)
    if tgt == shp:
        return x
    low = ops.downsample_seg_nearest(x[None, None].contiguous(), tgt)
    return _zoom3(low, shp, planar=planar and tgt[0] == shp[0])[0, 0]


class SimulateLowResolutionDevice:
    """SimulateLowResolutionTransform(zoom_range=(0.5, 1), per_channel=True, p_per_channel=0.5, order_downsample=0,
    order_upsample=3, p_per_sample=0.25, ignore_axes) (data_augmentation_moreDA.py:100-103)."""

    def __init__(self, zoom_range=(0.5, 1), per_channel=True, p_per_channel=0.5, p_per_sample=0.25, ignore_axes=None):
        self.zoom, self.per_channel, self.ppc, self.p, self.ignore = zoom_range, per_channel, p_per_channel, p_per_sample, ignore_axes

    def __call__(self, data):
        shp = np.array([int(i) for i in data.shape[2:]])
        planar = self.ignore is not None and tuple(self.ignore) == (0,)
        for b in range(data.shape[0]):
            if np.random.uniform() < self.p:
                target = None
                if not self.per_channel:
                    target = np.round(shp * np.random.uniform(self.zoom[0], self.zoom[1])).astype(int)
                for c in range(data.shape[1]):
                    if np.random.uniform() < self.ppc:
                        if self.per_channel:
                            target = np.round(shp * np.random.uniform(self.zoom[0], self.zoom[1])).astype(int)
                        t = target.copy()
                        if self.ignore is not None:
                            for i in self.ignore:
                                t[i] = shp[i]
                        data[b, c] = simulate_low_resolution_device(data[b, c], t, planar)
        return data


def _intensity_batch(data, params, who):
    """The checks the three functional forms share -> (parameters as float64 [N, C], mask of the channels to change)."""
    from ... import ops
    ops._require_device(ops._AUG, data)
    if data.dim() != 5 or data.dtype != torch.float32:
        raise ValueError("%s: a float32 [N, C, D, H, W] batch is expected, got %s %s" % (who, data.dtype, tuple(data.shape)))
    N, C = int(data.shape[0]), int(data.shape[1])
    params = np.asarray(params, dtype=np.float64)
    if params.shape != (N, C):
        raise ValueError("%s: parameters of shape %s for a batch of %d x %d channels" % (who, params.shape, N, C))
    return params, ~np.isnan(params)


def _records(on, op, a, flags=0, b=0.):
    from ... import ops
    rec = np.zeros(on.size, dtype=ops.INTENSITY_OP_DTYPE)           # op 0: the channel is neither read nor written
    on = on.reshape(-1)
    rec['op'][on], rec['flags'][on], rec['b'][on] = op, flags, b
    rec['a'][on] = a.reshape(-1)[on]
    return rec


def _in_place(data, fn):
    """fn on data itself, or on a contiguous copy that is copied back."""
    work = data if data.is_contiguous() else data.contiguous()
    fn(work)
    if work is not data:
        data.copy_(work)
    return data


def augment_brightness_device(data, multipliers):
    """data[n, c] *= multipliers[n, c] in place on a [N, C, D, H, W] float32 device batch; multipliers: [N, C] host array, NaN
    leaves that channel alone.  One launch (`mt_intensity_apply`); returns data."""
    from ... import ops
    m, on = _intensity_batch(data, multipliers, 'augment_brightness_device')
    if not on.any():
        return data
    return _in_place(data, lambda x: ops.intensity_apply(x, _records(on, ops.INTENSITY_SCALE, m)))


def augment_contrast_device(data, factors, preserve_range=True):
    """batchgenerators' augment_contrast for every (sample, channel) with its own factor, in place: x = (x - mean) * f + mean, then
    clipped to the channel's own [min, max] when preserve_range.  factors: [N, C] host array, NaN leaves that channel alone.  Two
    launches for the statistics (`mt_channel_stats`), one for the pass (`mt_intensity_apply`); nothing is read back.  Returns data."""
    from ... import ops
    f, on = _intensity_batch(data, factors, 'augment_contrast_device')
    if not on.any():
        return data
    rec = _records(on, ops.INTENSITY_CONTRAST, f, ops.INTENSITY_PRESERVE_RANGE if preserve_range else 0)
    return _in_place(data, lambda x: ops.intensity_apply(x, rec, ops.channel_stats(x, on)))


def augment_gamma_device(data, gammas, invert=False, retain_stats=True, epsilon=1e-7):
    """batchgenerators' augment_gamma for every (sample, channel) with its own gamma, in place: on y = -x when invert, else x,
    y = ((y - min) / (max - min + epsilon))^gamma * (max - min) + min, then with retain_stats y = (y - mean') / (sd' + 1e-8) * sd + mean
    (mean, sd before and mean', sd' after the power), and -y is stored when invert.  gammas: [N, C] host array, NaN leaves that channel
    alone.  statistics -> power (-> statistics -> restore) on `mt_channel_stats` / `mt_intensity_apply`; nothing is read back.
    Returns data."""
    from ... import ops
    g, on = _intensity_batch(data, gammas, 'augment_gamma_device')
    if not on.any():
        return data
    rec = _records(on, ops.INTENSITY_GAMMA, g, ops.INTENSITY_NEGATE if invert else 0, epsilon)

    def run(x):
        before = ops.channel_stats(x, on)
        ops.intensity_apply(x, rec, before)
        if retain_stats:
            rec['op'][on.reshape(-1)] = ops.INTENSITY_RESTORE
            ops.intensity_apply(x, rec, before, ops.channel_stats(x, on))
    return _in_place(data, run)


class _IntensityTransform:
    """What the three transforms share.  plan(N, C) makes ALL numpy draws of a batch, in batchgenerators' order, and returns the
    drawn parameter per statistics group as a float64 array, NaN where nothing was drawn: [N, C] with per_channel, else [N, 1] (one
    parameter and one set of statistics for the C * V elements of a sample).  __call__ then issues one launch group for the batch
    on the [N, 1, C * D, H, W] view of the same memory in the second case; with nothing drawn, nothing is launched."""

    def _draw(self):
        raise NotImplementedError

    def _apply(self, data, params):
        raise NotImplementedError

    def plan(self, N, C):
        G = C if self.per_channel else 1
        params = np.full((N, G), np.nan)
        for b in range(N):
            if np.random.uniform() < self.p:
                for c in range(G):
                    params[b, c] = self._draw()
        return params

    def __call__(self, data):
        from ... import ops
        ops._require_device(ops._AUG, data)
        N, C = int(data.shape[0]), int(data.shape[1])
        params = self.plan(N, C)
        if np.isnan(params).all():
            return data
        if params.shape[1] == C:
            return self._apply(data, params)
        return _in_place(data, lambda x: self._apply(x.view(N, 1, C * int(x.shape[2]), int(x.shape[3]), int(x.shape[4])), params))


class BrightnessMultiplicativeDevice(_IntensityTransform):
    def __init__(self, multiplier_range=(0.75, 1.25), per_channel=True, p_per_sample=0.15):
        self.r, self.per_channel, self.p = multiplier_range, per_channel, p_per_sample

    def _draw(self):
        return np.random.uniform(self.r[0], self.r[1])

    def _apply(self, data, params):
        return augment_brightness_device(data, params)


class ContrastAugmentationDevice(_IntensityTransform):
    def __init__(self, contrast_range=(0.75, 1.25), preserve_range=True, per_channel=True, p_per_sample=0.15):
        self.r, self.preserve, self.per_channel, self.p = contrast_range, preserve_range, per_channel, p_per_sample

    def _draw(self):
        return _range_pick(self.r[0], self.r[1])

    def _apply(self, data, params):
        return augment_contrast_device(data, params, bool(self.preserve))


class GammaDevice(_IntensityTransform):
    def __init__(self, gamma_range=(0.7, 1.5), invert_image=False, per_channel=True, retain_stats=True, p_per_sample=0.3, epsilon=1e-7):
        self.r, self.invert, self.per_channel, self.retain, self.p, self.eps = gamma_range, invert_image, per_channel, retain_stats, p_per_sample, epsilon

    def _draw(self):
        return _range_pick(self.r[0], self.r[1])

    def _apply(self, data, params):
        return augment_gamma_device(data, params, bool(self.invert), bool(self.retain), self.eps)


class MaskTransformDevice:
    """batchgenerators MaskTransform(dct_for_where_it_was_used, mask_idx_in_seg=0, set_outside_to=0)
    (data_augmentation_moreDA.py:113-115): every channel c with dct[c] true is set to `set_outside_to` where
    seg[b, mask_idx_in_seg] < 0, i.e. outside the non-zero mask the preprocessing normalised in (use_mask_for_norm).  Elementwise
    torch glue on whatever device the tensors live on; in place like the reference."""

    def __init__(self, dct_for_where_it_was_used, mask_idx_in_seg=0, set_outside_to=0):
        self.dct, self.seg_idx, self.outside = dict(dct_for_where_it_was_used), mask_idx_in_seg, set_outside_to

    def __call__(self, data, seg):
        channels = [int(c) for c, used in self.dct.items() if used]
        if not channels:
            return data
        if seg is None:
            raise ValueError("MaskTransform needs the segmentation: its label -1 marks the outside of the non-zero mask")
        outside = seg[:, self.seg_idx] < 0
        for c in channels:
            data[:, c].masked_fill_(outside, self.outside)
        return data


class MoreDADeviceAugmenter:
    """DataLoader3D batches (loader patch = basic_generator_patch_size) -> device -> SpatialTransform (with elastic deformation
    when params["do_elastic"]) -> noise, blur, brightness, contrast, simulated low resolution, gamma (inverted), gamma -> mirror ->
    MaskTransform (when params carries "mask_was_used_for_normalization") -> {'data', 'target' (one label map; the trainers build
    the pyramid and remove label -1 on the device), 'properties', 'keys'}: get_moreDA_augmentation's order
    (data_augmentation_moreDA.py:41-153) without the cascade transforms and the CPU worker pool."""

    def __init__(self, loader, patch_size, params, device, border_val_seg=-1, order_seg=1, order_data=3):
        from .spatial import MirrorTransformDevice, SpatialTransformDevice
        self.loader, self.device = loader, device
        self.spatial = SpatialTransformDevice(
            patch_size, patch_center_dist_from_border=None, do_elastic_deform=params.get("do_elastic"),
            do_rotation=params.get("do_rotation"), angle_x=params.get("rotation_x"), angle_y=params.get("rotation_y"),
            angle_z=params.get("rotation_z"), p_rot_per_axis=params.get("rotation_p_per_axis"), do_scale=params.get("do_scaling"),
            scale=params.get("scale_range"), border_mode_data=params.get("border_mode_data"), border_cval_data=0, order_data=order_data,
            border_mode_seg="constant", border_cval_seg=border_val_seg, order_seg=order_seg, random_crop=params.get("random_crop"),
            p_el_per_sample=params.get("p_eldef"), p_scale_per_sample=params.get("p_scale"), p_rot_per_sample=params.get("p_rot"),
            independent_scale_for_each_axis=params.get("independent_scale_factor_for_each_axis"), dummy_2d=bool(params.get("dummy_2D")),
            alpha=params.get("elastic_deform_alpha"), sigma=params.get("elastic_deform_sigma"))
        ignore_axes = (0,) if params.get("dummy_2D") else None               # data_augmentation_moreDA.py:55-64
        self.color = [GaussianNoiseDevice(p_per_sample=0.1),
                      GaussianBlurDevice((0.5, 1.), different_sigma_per_channel=True, p_per_sample=0.2, p_per_channel=0.5),
                      BrightnessMultiplicativeDevice((0.75, 1.25), p_per_sample=0.15),
                      ContrastAugmentationDevice(p_per_sample=0.15),
                      SimulateLowResolutionDevice((0.5, 1), per_channel=True, p_per_channel=0.5, p_per_sample=0.25, ignore_axes=ignore_axes),
                      GammaDevice(params.get("gamma_range"), True, True, params.get("gamma_retain_stats"), 0.1)]
        if params.get("do_gamma"):
            self.color.append(GammaDevice(params.get("gamma_range"), False, True, params.get("gamma_retain_stats"), params["p_gamma"]))
        self.mirror = MirrorTransformDevice(params.get("mirror_axes")) if params.get("do_mirror") else None
        used = params.get("mask_was_used_for_normalization")
        self.mask = MaskTransformDevice(used, mask_idx_in_seg=0, set_outside_to=0) if used is not None else None

    def __iter__(self):
        return self

    def __next__(self):
        b = next(self.loader)
        if torch.is_tensor(b['data']):                      # DeviceDataLoader3D: the batch is on the device already
            data, seg = b['data'].to(self.device), b['seg'][:, :1].to(self.device)
        else:
            data = torch.from_numpy(b['data']).to(self.device, non_blocking=True)
            seg = torch.from_numpy(b['seg'][:, :1]).to(self.device, non_blocking=True)
        data, seg = self.spatial(data, seg)
        for t in self.color:
            data = t(data)
        if self.mirror is not None:
            data, seg = self.mirror(data, seg)
        if self.mask is not None:
            data = self.mask(data, seg)
        return {'data': data, 'target': seg, 'properties': b['properties'], 'keys': b['keys']}


def default_3d_augmentation_params():
    """default_3D_augmentation_params (default_data_augmentation.py:39-92) with nnUNetTrainerV2.setup_DA_params's overrides
    (nnUNetTrainerV2.py:352-389): rotations +-30 degrees, scale (0.7, 1.4), no elastic deformation (its alpha / sigma ranges are
    the reference's 3D defaults for a trainer that turns it on)."""
    r = 30. / 360 * 2. * np.pi
    return {"do_elastic": False, "elastic_deform_alpha": (0., 900.), "elastic_deform_sigma": (9., 13.), "p_eldef": 0.2, "do_scaling": True, "scale_range": (0.7, 1.4),
            "independent_scale_factor_for_each_axis": False, "p_scale": 0.2, "do_rotation": True, "rotation_x": (-r, r),
            "rotation_y": (-r, r), "rotation_z": (-r, r), "rotation_p_per_axis": 1, "p_rot": 0.2, "random_crop": False,
            "do_gamma": True, "gamma_retain_stats": True, "gamma_range": (0.7, 1.5), "p_gamma": 0.3, "do_mirror": True,
            "mirror_axes": (0, 1, 2), "dummy_2D": False, "border_mode_data": "constant"}
