"""mt_softmax_dice_ce_fwd / _bwd beyond 16 classes (the wave-per-voxel kernels, 17..64 classes: Task100's 47 labels through a softmax
trainer give 48) against float64 torch on the host: the statistics (ce_sum, tp, fp, fn) of dice_loss.py:100-195 / crossentropy.py:4-11
and, for random dLoss/dstats, the gradient autograd gives for sum(gstats * stats).  16 classes, the widest case of the register
kernels, runs beside them through the same comparison.

Tolerances: a statistic is a float32 sum of at most 1024 terms in [0, 1] per block (then summed in float64), so its error is below
1024 * 2^-24 = 6.1e-5 of its value, plus a few ulp of __expf / __logf per term; 1e-4 relative (and the same absolute for sums near 0)
bounds that.  A gradient element is a handful of float32 operations on numbers of the size of `scale` = max |gstats|: 1e-5 * scale."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPE = (5, 13, 21)          # 1365 voxels: a whole block of 1024 and a partial one, an odd count per wave


def _case(C, cs, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2
    buf = torch.randn((B,) + SHAPE + (cs,), generator=g) * 3.0
    target = torch.randint(0, C, (B, 1) + SHAPE, generator=g).float()
    target[0, 0, 0, 0, :5] = torch.tensor([0.0, C - 1.0, 1.0, C - 1.0, 0.0])
    gstats = torch.randn((B, C, 4), generator=g)
    return buf, target, gstats


def _reference(x64, target, gstats):
    """x64: [B, V, C] float64 leaf -> (stats [B, C, 4], d sum(gstats * stats) / dx); only slot (b, 0, 0) of the CE column counts."""
    B, V, C = x64.shape
    p = torch.softmax(x64, dim=2)
    y = torch.nn.functional.one_hot(target.reshape(B, V).long(), C).double()
    tp, fp, fn = (p * y).sum(1), (p * (1 - y)).sum(1), ((1 - p) * y).sum(1)
    ce = -(torch.log(p) * y).sum((1, 2))
    stats = torch.zeros((B, C, 4), dtype=torch.float64)
    stats = torch.stack([torch.cat([ce[:, None], torch.zeros(B, C - 1, dtype=torch.float64)], 1), tp, fp, fn], dim=2)
    g = gstats.double().clone()
    g[:, 1:, 0] = 0
    (stats * g).sum().backward()
    return stats.detach(), x64.grad


@pytest.mark.parametrize('C,cs', [(16, 16), (17, 17), (48, 48), (48, 50), (64, 64)])
def test_softmax_statistics_and_gradient_against_float64(dev, C, cs):
    from multitalent_amd import ops
    from multitalent_amd.ops import Act
    buf, target, gstats = _case(C, cs, 100 + C + cs)
    B, V = buf.shape[0], int(np.prod(SHAPE))
    x64 = buf[..., :C].reshape(B, V, C).double().requires_grad_(True)
    want, dwant = _reference(x64, target, gstats)
    a = Act(buf.to(dev), c0=0, C=C)
    stats = torch.full((B, C, 4), float('nan'), dtype=torch.float32, device=dev)
    ws = torch.empty(ops.loss_workspace(B, V, C) // 4 + 1, dtype=torch.float32, device=dev)
    ops.softmax_dice_ce_fwd(a, target.to(dev), stats, ws)
    got = stats.cpu().double()
    got[:, 1:, 0] = 0                                            # only the c = 0 slot of the CE column is defined
    err = (got - want).abs()
    assert bool((err <= 1e-4 * want.abs() + 1e-4).all()), float(err.max())
    d = torch.full(buf.shape, 7.0, dtype=torch.float32, device=dev)
    ops.softmax_dice_ce_bwd(a, target.to(dev), gstats.to(dev), Act(d, c0=0, C=C))
    dgot = d.cpu()
    assert bool((dgot[..., C:] == 7.0).all())                    # channels beyond C of a wider buffer are not written
    scale = float(gstats.abs().max())
    derr = float((dgot[..., :C].reshape(B, V, C).double() - dwant).abs().max())
    assert derr <= 1e-5 * scale, (derr, scale)
    again = torch.empty_like(stats)
    ops.softmax_dice_ce_fwd(a, target.to(dev), again, ws)
    assert torch.equal(again[:, :, 1:], stats[:, :, 1:]) and torch.equal(again[:, 0, 0], stats[:, 0, 0])       # run to run


def test_softmax_loss_rejects_more_than_64_classes(dev):
    from multitalent_amd import ops
    from multitalent_amd.ops import Act
    buf = torch.zeros((1, 2, 2, 2, 65), device=dev)
    with pytest.raises(RuntimeError, match='2 <= C <= 64'):
        ops.softmax_dice_ce_fwd(Act(buf), torch.zeros((1, 1, 2, 2, 2), device=dev), torch.zeros((1, 65, 4), device=dev),
                                torch.zeros(4096, device=dev))


@pytest.mark.parametrize('batch_dice', [False, True])
def test_48_class_fused_step_matches_the_autograd_form(dev, batch_dice):
    """DC_and_CE_DS_loss as nnUNetTrainerV2 builds it, 48 classes over three levels: value and dLoss/dlogits of fused_step against
    the autograd spelling (the comparison and bound of tests/test_loss_combine_gpu.py)."""
    from multitalent_amd.training.loss_functions.fused_losses import DC_and_CE_DS_loss
    shapes = [(8, 24, 24), (4, 12, 12), (2, 6, 6)]
    C, B = 48, 2
    g = torch.Generator().manual_seed(48)
    outs = [(torch.randn((B,) + s + (C,), generator=g) * 2.0).to(dev) for s in shapes]
    target = [torch.randint(0, C, (B, 1) + s, generator=g).float().to(dev) for s in shapes]
    loss_fn = DC_and_CE_DS_loss([0.5, 0.3, 0.2], batch_dice=batch_dice)
    leaves = [o.permute(0, 4, 1, 2, 3).requires_grad_(True) for o in outs]
    res = loss_fn(leaves, target)
    (res[0] if isinstance(res, tuple) else res).backward()
    fused = loss_fn.fused_step(outs, target)
    assert fused is not None
    fa = [float(r) for r in (res if isinstance(res, tuple) else (res,))]
    ff = [float(r) for r in (fused[0] if isinstance(fused[0], tuple) else (fused[0],))]
    assert np.allclose(ff, fa, rtol=2e-6, atol=2e-6), (ff, fa)
    for a, leaf in zip(fused[1], leaves):
        b = leaf.grad.permute(0, 2, 3, 4, 1).contiguous()
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-6 * scale + 1e-12
