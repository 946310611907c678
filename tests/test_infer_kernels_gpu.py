"""The prediction path on real memory against float64: every instance of the fused inference heads (csrc/head_infer.hip), the five
kernels of csrc/infer.hip and the driver predict_3D.  Cases, references and bounds are tests/infer_cases.py (see its docstring);
tests/test_infer_cases_cpu.py checks the references and shows what the cases reach.  Operands are channel slices of wider allocations
whose other channels hold the largest finite value; destinations that are assigned start as NaN, destinations that are accumulated
into start from seeded contents, every destination lies between guard elements; after a launch the sources are bit-identical, nothing
outside the destination has changed and no NaN is left inside.  Every figure is printed before it is asserted."""
import ctypes as Ct
import functools
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import infer_cases as IC
import mask_check

pytestmark = pytest.mark.gpu

IDS = lambda c: c.id if hasattr(c, 'id') else c[0]


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib, ops
    return dev, _lib.load(), _lib, ops


def stops_on_hip_error(fn):
    """A HIP error ends the whole run: nothing more is launched on a device that has faulted (as test_kernel_instances_gpu._run)."""
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


def _bits(t):
    iv = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]
    return t.contiguous().view(iv)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Guarded(object):
    """a destination between IC.GUARD sentinels on each side: .view is the device tensor the kernel gets"""

    def __init__(self, dev, host, sentinel=IC.SENTINEL):
        self.shape, self.n = tuple(host.shape), host.numel()
        pad = torch.full((IC.GUARD,), sentinel, dtype=host.dtype)
        self.host = torch.cat([pad, host.reshape(-1), pad])
        self.dev = self.host.to(dev)
        self.view = self.dev[IC.GUARD:IC.GUARD + self.n].view(self.shape)

    def fetch(self):
        after = self.dev.cpu()
        assert _same_bits(after[:IC.GUARD], self.host[:IC.GUARD]) and _same_bits(after[-IC.GUARD:], self.host[-IC.GUARD:]), \
            "guard elements around a destination changed"
        return after[IC.GUARD:IC.GUARD + self.n].view(self.shape)


def _nan(*shape):
    return torch.full(shape, float('nan'))


def _fig(kernel, case_id, what, value):
    print('INFER-FIG %s %s %s %.3e' % (kernel, case_id, what, value))


def _outside_unchanged(after, before, box):
    """everything of `after` outside the box (slices over the LAST three axes) is bit-identical to `before`"""
    m = torch.ones(after.shape, dtype=torch.bool)
    m[(Ellipsis,) + tuple(box)] = False
    return torch.equal(_bits(after)[m], _bits(before)[m])


# ================================================================================================================================
@pytest.mark.parametrize('case', IC.head_cases(), ids=IDS)
@stops_on_hip_error
def test_fused_head_instance(env, case):
    dev, lib, _lib, ops = env
    c, d = case, IC.head_draw(case)
    N, shape = IC.head_N(c), c.shape
    buf = IC.head_buffer(c, d)
    bufd = buf.to(dev)
    assert bufd.data_ptr() % 256 == 0
    sc, sh = (d['scale'].to(dev).contiguous(), d['shift'].to(dev).contiguous()) if c.aff else (None, None)
    xa = ops.Act(bufd, c0=c.c0, C=c.cin, scale=sc, shift=sh, slope=c.slope)
    wd = d['w'].to(dev).contiguous()
    wp = ops.pack_conv_weights(wd, c.cin, 0, c.cout, (1, 1, 1), ops.conv_weight_strides(wd), False, ops.POINTWISE_CK)
    bd = d['b'].to(dev) if c.bias else None
    unused = torch.empty((N,) + shape + (c.cout,), device=dev)
    p = ops.fill_pointwise(xa, shape, shape, (1, 1, 1), (1, 1, 1), c.cout, wp, bd, ops.Act(unused))
    pred = IC.head_pred(c, d)

    # ---- mt_head_flip_accumulate: first = 1 into NaN, then first = 0 on top
    assert ops.head_infer_kernel_name(p, False) == IC.head_name(c, False)
    acc = Guarded(dev, _nan(c.cout, *shape))
    one, two = IC.head_flip_ref(c, pred)
    ops.head_flip_accumulate(p, c.fsamples[0], IC.bits(c.fflips[0]), c.nonlin, c.fweights[0], acc.view, True)
    torch.cuda.synchronize()
    got1 = acc.fetch().clone()
    ops.head_flip_accumulate(p, c.fsamples[1], IC.bits(c.fflips[1]), c.nonlin, c.fweights[1], acc.view, False)
    torch.cuda.synchronize()
    got2 = acc.fetch()
    assert _same_bits(bufd.cpu(), buf), "head_flip_accumulate changed its source"
    assert not torch.isnan(got1).any() and not torch.isnan(got2).any()
    e1, e2 = IC.relerr(got1, one), IC.relerr(got2, two)
    _fig('head_flip_accumulate', c.id, 'relerr', max(e1, e2))
    assert e1 < IC.HEAD_BOUND and e2 < IC.HEAD_BOUND, (e1, e2)

    # ---- mt_head_mirror_accumulate: every sample of the tile into the aggregate's prior contents
    assert ops.head_infer_kernel_name(p, True) == IC.head_name(c, True)
    adims, origin = IC.head_agg_geometry(c)
    agg = Guarded(dev, d['agg0'])
    nb = Guarded(dev, d['nb0']) if c.nb else None
    gs = d['gauss'].to(dev) if c.gauss else None
    ops.head_mirror_accumulate(p, c.sample0, [IC.bits(f) for f in c.flips], c.nonlin, IC.head_mirror_weight(c), gs,
                               agg.view, nb.view if nb else None, adims, origin)
    torch.cuda.synchronize()
    want, wnb = IC.head_mirror_ref(c, d, pred)
    got = agg.fetch()
    box = tuple(slice(o, o + s) for o, s in zip(origin, shape))
    assert _same_bits(bufd.cpu(), buf), "head_mirror_accumulate changed its source"
    assert _outside_unchanged(got, d['agg0'], box), "head_mirror_accumulate wrote outside its tile"
    assert not torch.isnan(got).any()
    e = IC.relerr(got, want)
    _fig('head_mirror_accumulate', c.id, 'relerr', e)
    assert e < IC.HEAD_BOUND, e
    if nb is not None:
        assert torch.equal(nb.fetch(), wnb), "nb is one fp32 addition per voxel"
    if gs is not None:
        assert _same_bits(gs.cpu(), d['gauss'])


# ================================================================================================================================
@pytest.mark.parametrize('case', IC.flipacc_cases(), ids=IDS)
@stops_on_hip_error
def test_flip_accumulate(env, case):
    dev, lib, _lib, ops = env
    c, d = case, IC.flipacc_draw(case)
    bufd = d['buf'].to(dev)
    la = ops.Act(bufd, c0=c.c0, C=c.C)
    acc = Guarded(dev, _nan(c.C, *c.shape))
    one, two = IC.flipacc_ref(c, d)
    ops.flip_accumulate(la, IC.bits(c.code), c.nonlin, c.weights[0], acc.view, True)
    torch.cuda.synchronize()
    got1 = acc.fetch().clone()
    ops.flip_accumulate(la, IC.bits(c.code), c.nonlin, c.weights[1], acc.view, False)
    torch.cuda.synchronize()
    got2 = acc.fetch()
    assert _same_bits(bufd.cpu(), d['buf']), "flip_accumulate changed its source"
    assert not torch.isnan(got1).any() and not torch.isnan(got2).any()
    e1, e2 = IC.relerr(got1, one), IC.relerr(got2, two)
    _fig('flip_accumulate', c.id, 'relerr', max(e1, e2))
    assert e1 < IC.HEAD_BOUND and e2 < IC.HEAD_BOUND, (e1, e2)
    if IC.flipacc_exact(c):
        assert _same_bits(got1, one.float()), "nonlin 0, a power-of-two weight, first = 1: bit-equal"


@stops_on_hip_error
def test_flip_accumulate_refuses_160_classes(env):
    dev, lib, _lib, ops = env
    buf = torch.zeros((1, 1, 2, 3, 160), device=dev)
    acc = Guarded(dev, _nan(160, 1, 2, 3))
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        ops.flip_accumulate(ops.Act(buf), (False, False, False), 0, 1.0, acc.view, True)
    torch.cuda.synchronize()
    assert torch.isnan(acc.fetch()).all(), "refused without a launch"


# ================================================================================================================================
@pytest.mark.parametrize('case', IC.extract_cases(), ids=IDS)
@stops_on_hip_error
def test_extract_tiles(env, case):
    dev, lib, _lib, ops = env
    cid, Cn, vdims, patch, tiles = case
    vol = torch.randn((Cn,) + vdims, generator=IC.gen('extract', cid))
    vold = vol.to(dev)
    out = Guarded(dev, _nan(len(tiles), Cn, *patch))
    ops.extract_tiles(vold, patch, [(o, IC.bits(code)) for o, code in tiles], out.view)
    torch.cuda.synchronize()
    assert _same_bits(out.fetch(), IC.extract_ref(vol, patch, tiles)) and _same_bits(vold.cpu(), vol)


@stops_on_hip_error
def test_extract_tiles_refusals(env):
    dev, lib, _lib, ops = env
    vol = torch.zeros((1, 6, 7, 9), device=dev)
    out = Guarded(dev, _nan(65, 1, 2, 3, 4))
    none = (False, False, False)
    with pytest.raises(RuntimeError, match=r'rc=-1'):
        ops.extract_tiles(vol, (2, 3, 4), [((0, 0, 0), none)] * 65, out.view)
    for o in ((5, 0, 0), (0, 5, 0), (0, 0, 6), (-1, 0, 0)):
        with pytest.raises(RuntimeError, match=r'rc=-1'):
            ops.extract_tiles(vol, (2, 3, 4), [((0, 0, 0), none), (o, none)], out.view[:2])
    torch.cuda.synchronize()
    assert torch.isnan(out.fetch()).all()


# ================================================================================================================================
@pytest.mark.parametrize('case', IC.tile_cases(), ids=IDS)
@stops_on_hip_error
def test_tile_accumulate(env, case):
    dev, lib, _lib, ops = env
    c, d = case, IC.tile_draw(case)
    accd = d['acc'].to(dev)
    gs = d['gauss'].to(dev) if c.gauss else None
    agg = Guarded(dev, d['agg0'])
    nb = Guarded(dev, d['nb0']) if c.nb else None
    ops.tile_accumulate(accd, gs, c.C, c.patch, agg.view, nb.view if nb else None, c.adims, c.origin)
    torch.cuda.synchronize()
    want, wnb = IC.tile_ref(c, d)
    got = agg.fetch()
    box = tuple(slice(o, o + s) for o, s in zip(c.origin, c.patch))
    assert _same_bits(accd.cpu(), d['acc']) and (gs is None or _same_bits(gs.cpu(), d['gauss']))
    assert _outside_unchanged(got, d['agg0'], box) and not torch.isnan(got).any()
    e = IC.relerr(got, want)
    _fig('tile_accumulate', c.id, 'relerr', e)
    assert e <= IC.TILE_BOUND, e
    if nb is not None:
        assert torch.equal(nb.fetch(), wnb)


@stops_on_hip_error
def test_tile_accumulate_refused_outside_the_aggregate(env):
    dev, lib, _lib, ops = env
    acc = torch.ones((2, 3, 4, 5), device=dev)
    agg = Guarded(dev, torch.zeros(2, 4, 5, 6))
    for o in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (0, -1, 0)):
        with pytest.raises(RuntimeError, match=r'rc=-1'):
            ops.tile_accumulate(acc, None, 2, (3, 4, 5), agg.view, None, (4, 5, 6), o)
    torch.cuda.synchronize()
    assert not agg.fetch().any()


# ================================================================================================================================
@pytest.mark.parametrize('case', IC.norm_cases(), ids=IDS)
@stops_on_hip_error
def test_normalize_threshold(env, case):
    dev, lib, _lib, ops = env
    c, d = case, IC.norm_draw(case)
    agg = Guarded(dev, d['agg'])
    nbd = d['nb'].to(dev) if c.nb else None
    seg = Guarded(dev, torch.full((c.V,), -77, dtype=torch.int32), sentinel=-5) if c.seg else None
    order = torch.tensor(c.order, dtype=torch.int32, device=dev) if c.order is not None else None
    ops.normalize_threshold(agg.view, nbd, c.C, c.V, order, c.order is not None, seg.view if seg else None)
    torch.cuda.synchronize()
    probs = agg.fetch().numpy()
    assert nbd is None or _same_bits(nbd.cpu(), d['nb'])
    assert not np.isnan(probs).any()
    q = d['agg'].double().numpy() / (d['nb'].double().numpy() if c.nb else 1.0)
    ulps = np.abs(probs.astype(np.float64) - q) / np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
    _fig('normalize_threshold', c.id, 'ulps', float(ulps.max()))
    assert ulps.max() <= 1.0
    assert (probs == 0.5).any()
    if seg is not None:
        got = seg.fetch().numpy()
        assert np.array_equal(got.astype(np.int64), IC.decide_ref(probs, c.order)), "seg is not the rule applied to the returned probabilities"


# ================================================================================================================================
def _resample(lib, _lib, probs, c, out, order):
    rc = lib.mt_resample_classify(Ct.c_void_p(probs.data_ptr()), c.C, c.ishape[0], c.ishape[1], c.ishape[2], c.oshape[0], c.oshape[1],
                                  c.oshape[2], c.sep, Ct.c_void_p(order.data_ptr()) if order is not None else None,
                                  int(order is not None), Ct.c_void_p(out.data_ptr()), c.full[0], c.full[1], c.full[2],
                                  c.off[0], c.off[1], c.off[2], Ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'resample_classify ' + c.id)


@pytest.mark.parametrize('case', IC.resample_cases(), ids=IDS)
@stops_on_hip_error
def test_resample_classify(env, case):
    dev, lib, _lib, ops = env
    c = case
    probs = IC.rs_probs(c)
    pd = probs.to(dev)
    before = torch.full(c.full, 201, dtype=torch.uint8)
    out = Guarded(dev, before, sentinel=77)
    order = torch.tensor(c.order, dtype=torch.int32, device=dev) if c.order is not None else None
    _resample(lib, _lib, pd, c, out.view, order)
    torch.cuda.synchronize()
    got = out.fetch()
    sl, box = IC.resample_box(c)
    assert _same_bits(pd.cpu(), probs) and _outside_unchanged(got, before, sl), "resample_classify wrote outside its box"
    vals = IC.resample_values(probs.numpy(), c.oshape, c.sep)[(slice(None),) + box]
    left_out = IC.resample_excluded(vals, c.order)
    _fig('resample_classify', c.id, 'excluded_share', float(left_out.mean()))
    assert left_out.mean() < IC.RS_MAX_OUT
    want = IC.decide_ref(vals, c.order)
    g = got[sl].numpy().astype(np.int64)
    assert np.array_equal(g[~left_out], want[~left_out])
    labels = set(c.order) | {0} if c.order is not None else set(range(c.C))
    assert set(np.unique(g).tolist()) <= labels


@stops_on_hip_error
def test_resample_classify_stride_loop(env):
    """more than 65536 blocks of 256 output voxels; the float64 restatement runs as torch gathers on the device"""
    dev, lib, _lib, ops = env
    c = IC.RS_LARGE
    probs = IC.rs_probs(c)
    pd = probs.to(dev)
    out = torch.full((2 * IC.GUARD + int(np.prod(c.full)),), 201, dtype=torch.uint8, device=dev)
    view = out[IC.GUARD:-IC.GUARD].view(c.full)
    order = torch.tensor(c.order, dtype=torch.int32, device=dev)
    _resample(lib, _lib, pd, c, view, order)
    torch.cuda.synchronize()
    sl, box = IC.resample_box(c)
    assert int(np.prod([b.stop for b in box])) > 65536 * 256
    vals = IC.resample_values(pd, c.oshape, c.sep, xp=torch)[(slice(None),) + box][0]
    left_out = (vals - 0.5).abs() < IC.RS_MARGIN
    share = float(left_out.double().mean())
    _fig('resample_classify', c.id, 'excluded_share', share)
    assert share < IC.RS_MAX_OUT
    want = torch.where(vals > 0.5, c.order[0], 0).to(torch.uint8)
    got = view[sl]
    assert bool(((got == want) | left_out).all())
    m = torch.ones(c.full, dtype=torch.bool, device=dev)
    m[sl] = False
    assert bool((view[m] == 201).all()) and bool((out[:IC.GUARD] == 201).all()) and bool((out[-IC.GUARD:] == 201).all())
    assert _same_bits(pd.cpu(), probs)


# ================================================================================================================================
# the driver
PATCH, VOLUME = (8, 16, 16), (12, 24, 40)
_NETS = {}


def _net(dev, nc):
    """A small Generic_UNet as in test_golden_gpu, seeded.  mask_check caps the voxels within 1e-4 of a decision at 1 %, so the final
    head is set up to keep probabilities away from 0.5 without saturating them (a saturated sigmoid averages to k / 4 over four
    mirror combinations — exact ties): its weights are scaled to logits of unit spread over one random tile and its bias is +-2..3
    per class, so a class changes sides in about one voxel of a hundred."""
    from multitalent_amd.network_architecture.generic_UNet import Generic_UNet
    from multitalent_amd.network_architecture.initialization import InitWeights_He
    from multitalent_amd.utilities.nd_softmax import softmax_helper
    if nc not in _NETS:
        torch.manual_seed(100 + nc)
        pools, kernels = [[2, 2, 2], [1, 2, 2]], [[3, 3, 3]] * 3
        net = Generic_UNet(1, 6, nc, 2, 2, 2, nn.Conv3d, nn.InstanceNorm3d, {'eps': 1e-5, 'affine': True}, nn.Dropout3d,
                           {'p': 0, 'inplace': True}, nn.LeakyReLU, {'negative_slope': 1e-2, 'inplace': True}, True, False,
                           lambda x: x, InitWeights_He(1e-2), pools, kernels, False, True, True, seg_output_use_bias=True)
        net.to(dev)
        net.inference_apply_nonlin = softmax_helper if nc > 64 else nn.Sigmoid()
        net.eval()
        net.do_ds = False
        head = net.seg_outputs[-1]
        g = IC.gen('driver-net', nc)
        with torch.no_grad():
            head.bias.zero_()
            tile = torch.randn((1, 1) + PATCH, generator=g).to(dev)
            spread = float(net.engine().forward(tile, need_grad=False, all_heads=False)[0].std())
            k = 4.0 if nc > 64 else 1.0            # argmax of a softmax: saturation makes no ties, near-equal logits do
            head.weight.mul_(k / spread)
            sign = torch.where(torch.rand(nc, generator=g) < 0.5, -1.0, 1.0)
            head.bias.copy_((k * sign * (2.0 + torch.rand(nc, generator=g))).to(dev))
        net.engine().mark_params_dirty()
        _NETS[nc] = net
    return _NETS[nc]


def _order(nc):
    return None if nc > 64 else [int(v) for v in np.random.RandomState(nc).permutation(nc) + 1]


def _driver_reference(net, vol, dev, axes, gauss, nonlin):
    """float64 probabilities rebuilt from the engine's own logits of the same flipped tiles: nonlinearity, un-flip, mean over the mirror
    combinations, Gaussian, overlap-add in tile order (x, then y, then z), division (neural_network.py:287-428,502-591)"""
    from multitalent_amd.inference.sliding_window import compute_steps_for_sliding_window, get_gaussian
    steps = compute_steps_for_sliding_window(PATCH, vol.shape[1:], 0.5)
    tiles = list(itertools.product(*steps))
    assert len(tiles) > 8
    combos = [cmb for r in range(len(axes) + 1) for cmb in itertools.combinations(axes, r)]
    g = torch.from_numpy(get_gaussian(PATCH, 1. / 8)).double() if gauss else torch.ones(PATCH, dtype=torch.float64)
    v = torch.from_numpy(vol)
    samples = []
    for (x, y, z) in tiles:
        t = v[:, x:x + PATCH[0], y:y + PATCH[1], z:z + PATCH[2]]
        samples += [torch.flip(t, [a + 1 for a in cmb]) if cmb else t for cmb in combos]
    eng = net.engine()
    eng.set_precision('fp32')
    preds = []
    with torch.no_grad():
        for i in range(0, len(samples), 8):
            lg = eng.forward(torch.stack(samples[i:i + 8]).to(dev), need_grad=False, all_heads=False)[0]      # [B, D, H, W, C]
            torch.cuda.synchronize()
            preds += list(IC.nonlin_ref(lg.double().cpu().permute(0, 4, 1, 2, 3), nonlin, 1))
    agg = torch.zeros((net.num_classes,) + tuple(vol.shape[1:]), dtype=torch.float64)
    nb = torch.zeros(tuple(vol.shape[1:]), dtype=torch.float64)
    for ti, (x, y, z) in enumerate(tiles):
        s = sum(torch.flip(preds[ti * len(combos) + k], [a + 1 for a in cmb]) if cmb else preds[ti * len(combos) + k]
                for k, cmb in enumerate(combos)) / len(combos)
        agg[:, x:x + PATCH[0], y:y + PATCH[1], z:z + PATCH[2]] += s * g
        nb[x:x + PATCH[0], y:y + PATCH[1], z:z + PATCH[2]] += g
    return (agg / nb).numpy()


DRIVER = ([(nc, axes, gs) for nc in (5, 47) for axes in ((1, 2), (0,), ()) for gs in (True, False)] +
          [(70, (0, 1, 2), True), (70, (0,), False), (70, (), True), (70, (), False)])


@pytest.mark.parametrize('nc,axes,gauss', DRIVER, ids=['c%d-m%s-g%d' % (nc, ''.join(map(str, a)) or 'none', g) for nc, a, g in DRIVER])
@stops_on_hip_error
def test_predict_3d_against_its_own_logits(env, nc, axes, gauss):
    dev, lib, _lib, ops = env
    net, order = _net(dev, nc), _order(nc)
    vol = torch.randn((1,) + VOLUME, generator=IC.gen('driver', nc)).numpy()
    seg, probs = net.predict_3D(vol, do_mirroring=len(axes) > 0, mirror_axes=axes, use_sliding_window=True, step_size=0.5,
                                patch_size=PATCH, regions_class_order=order, use_gaussian=gauss, pad_border_mode='constant',
                                pad_kwargs={'constant_values': 0}, all_in_gpu=False, verbose=False, mixed_precision=False)
    ref = _driver_reference(net, vol, dev, axes, gauss, 2 if nc > 64 else 1)
    assert probs.shape == ref.shape and seg.shape == VOLUME
    e = float(np.abs(probs - ref).max())
    _fig('predict_3D', 'c%d-m%s-g%d' % (nc, ''.join(map(str, axes)) or 'none', gauss), 'max_abs_err', e)
    assert e < 1e-4
    ref_seg = mask_check.decide(ref, order)
    mask_check.check_masks(seg, ref_seg, probs, ref, order, 1e-4, 'predict_3D %d classes, mirror %r, gaussian %d' % (nc, axes, gauss), live=True)
