"""Case tables for multitalent_amd/engine.py: the part that composes the csrc kernels into a network.

  BRANCHES     every branch of engine.py that a valid network can reach, one tag each
  UNREACHABLE  branches that reading shows no valid network reaches, with the reason
  CONFIGS      small networks, each declaring the tags it `expects` (tests/test_engine_paths_gpu.py records which ran)
  SEQUENCES    call sequences on ONE engine and what each step is compared with (tests/test_engine_state_gpu.py)

plus the builders, the oracle call (oracle/reference_ops.py in fp32 / fp64) and compare(), the project's rule for a gradient.
numpy / torch on the CPU only: nothing here touches the device or loads libmtseg_hip.so (tests/test_engine_cases_cpu.py runs it all).

The fp32 oracle's own relative L2 gradient error against the fp64 oracle, per base configuration (seed 5 inputs; printed by
test_engine_cases_cpu.py::test_fp32_oracle_passes_compare, the figures are in DESIGN.md §6ah): 7e-7 .. 4.3e-6 — at these sizes the
reference itself is three orders of magnitude inside the 2e-3 global bound, so a failure on the device is the engine's.
"""
import numpy as np
import torch
from torch import nn

from oracle import reference_ops as R


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def build_plain(nc, base=10, pools=((2, 2, 2), (2, 2, 2), (1, 2, 2)), kernels=None, in_ch=1, max_num_features=None,
                seg_output_use_bias=False, internal_conv_bias=True):
    from multitalent_amd.network_architecture.generic_UNet import Generic_UNet
    from multitalent_amd.network_architecture.initialization import InitWeights_He
    pools = [list(p) for p in pools]
    kernels = [[3, 3, 3]] * (len(pools) + 1) if kernels is None else kernels
    torch.manual_seed(0)
    net = Generic_UNet(in_ch, base, nc, len(pools), 2, 2, nn.Conv3d, nn.InstanceNorm3d, {'eps': 1e-5, 'affine': True},
                       nn.Dropout3d, {'p': 0, 'inplace': True}, nn.LeakyReLU, {'negative_slope': 1e-2, 'inplace': True},
                       True, False, lambda x: x, InitWeights_He(1e-2), pools, kernels, False, True, True,
                       max_num_features=max_num_features, seg_output_use_bias=seg_output_use_bias, internal_conv_bias=internal_conv_bias)
    # make norm affine params and biases non-trivial
    g = torch.Generator().manual_seed(1)
    for n, p in net.named_parameters():
        if 'instnorm.weight' in n:
            p.data = 0.5 + torch.rand(p.shape, generator=g)
        elif n.endswith('bias'):
            p.data = 0.2 * torch.randn(p.shape, generator=g)
    return net, pools, kernels


RESENC_POOLS = [[1, 1, 1], [1, 2, 2], [2, 2, 2], [2, 2, 2]]
RESENC_KERNELS = [[1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]]
RESENC_BLOCKS = [1, 2, 2, 2]


def build_resenc(nc, base=8, blocks=RESENC_BLOCKS, pools=RESENC_POOLS, kernels=RESENC_KERNELS, in_ch=1, max_features=24, randomize=True, generator=None):
    """FabiansUNet as tests/test_network_gpu.py has always built it; randomize: non-trivial norm affine parameters and biases."""
    from multitalent_amd.network_architecture.generic_modular_residual_UNet import FabiansUNet, get_default_network_config
    from multitalent_amd.network_architecture.initialization import InitWeights_He
    pools, kernels, blocks = [list(p) for p in pools], [list(k) for k in kernels], list(blocks)
    torch.manual_seed(0)
    net = FabiansUNet(in_ch, base, blocks, 2, pools, kernels, get_default_network_config(3, None, norm_type="in"), nc, [1] * (len(pools) - 1),
                      True, False, max_features, InitWeights_He(1e-2))
    if randomize:
        g = torch.Generator().manual_seed(1) if generator is None else generator
        for n, p in net.named_parameters():
            if 'norm' in n and n.endswith('weight') and p.dim() == 1:
                p.data = 0.5 + torch.rand(p.shape, generator=g)
            elif n.endswith('bias'):
                p.data = 0.2 * torch.randn(p.shape, generator=g)
    return net, pools, kernels, blocks


def make_targets(shape, scales, nlabels, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    full = torch.randint(0, nlabels, (B, 1) + tuple(shape), generator=g).float()
    # blocky labels: nearest-neighbour upsample of a coarse grid
    coarse = torch.randint(0, nlabels, (B, 1) + tuple(max(s // 4, 1) for s in shape), generator=g).float()
    full = torch.nn.functional.interpolate(coarse, size=tuple(shape), mode='nearest')
    out = []
    for sc in scales:
        size = tuple(int(round(s * f)) for s, f in zip(shape, sc))
        out.append(torch.nn.functional.interpolate(full, size=size, mode='nearest'))
    return out


# ---- the project's rule for a gradient (moved unchanged from tests/test_fullsize_oracle_gpu.py) -----------------------------------------
ENTRY_BOUND = 0.03       # largest entry error of a gradient tensor, as a fraction of the tensor's largest exact entry


def compare(tag, logits, loss, grads, o32, o64, logit_tol=1e-3, loss_tol=1e-3):
    """Logits and loss: within 1e-3 of the fp32 oracle (north_star's tolerance; observed ~3e-5).
    Gradients: at this size the fp32 oracle ITSELF is 1e-3 .. 8e-3 (of a tensor's largest entry) away from the exact gradient:
    a LeakyReLU decision of a voxel within rounding of zero flips and changes that voxel's gradient hundredfold — at the 3x12x12
    stages one flipped voxel moves a weight-gradient entry by ~5 % of its typical size — and InstanceNorm backward subtracts means
    of 1.8 M-voxel sums.  So the truth is the fp64 oracle, and the HIP path is held to: per parameter tensor relative L2 error
    < 1e-2 (tensors whose exact gradient is not numerically zero), largest entry error < 0.03 max|g_64| + 1e-4 G (G = largest
    gradient entry of the network; the second term is the noise floor of gradients that are mathematically ZERO — the bias of every
    conv that feeds an InstanceNorm: 1e-19 in fp64, 1e-10 noise in both fp32 paths), globally relative L2 < max(2e-3, 1.6x the fp32
    torch oracle's own error) and 1 - cos < max(1e-5, 4x the oracle's).  (Round 5: tightened from 0.1 max|g| and max(5e-3, 2x); measured
    1.51e-3 against the oracle's 0.96e-3 on Task009, 0.87e-3 / 0.81e-3 on Task100, 5.0e-3 / 3.3e-3 on the residual encoder.)
    The HIP path normalises with ONE fma per element, t = y * (gamma rstd) + (beta - mu gamma rstd) (DESIGN.md §2 "lazy activations");
    rounding that per-channel offset to fp32 is a coherent 1-ulp perturbation: the same formula emulated inside the fp32 torch
    oracle raises ITS relative L2 gradient error from 0.9e-3 to 2.4e-3 (measured, Task009 network) — the HIP path measures 1.5e-3 on this test's batch (2.1e-3 on the batch of tools/diag_fullsize_grads.py)."""
    sd32, out32, l32 = o32
    sd64, out64, l64 = o64
    for i, (a, b) in enumerate(zip(logits, out32)):
        d = float((a - b.detach()).abs().max())
        assert d < logit_tol, "%s: logits of level %d differ by %.3e" % (tag, i, d)
    for a, b in zip(loss, l32):
        assert abs(a - float(b)) < loss_tol * max(1.0, abs(float(b))), (tag, loss, [float(r) for r in l32])
    G = max(float(v.grad.abs().max()) for v in sd64.values() if v.grad is not None)
    rows, ga, gt, gc = [], [], [], []
    for n, g in grads.items():
        t = sd64[n].grad
        if t is None:
            assert float(g.abs().max()) == 0.0, n           # e.g. the head of a zero-weight deep-supervision level
            continue
        c = sd32[n].grad.double()
        err, cerr, mx = float((g.double() - t).abs().max()), float((c - t).abs().max()), float(t.abs().max())
        # relative L2 only for tensors with a gradient worth the name (rms >= 1e-3 G): the norm biases of the 3x6x6 stage have
        # max|g| = 3e-4 G, and there 2e-5 G of backpropagated rounding noise is 6 % "relative" (r3: all five resenc outputs weighted)
        l2t = float((g.double() - t).norm() / t.norm()) if float(t.norm()) > 1e-3 * G * t.numel() ** 0.5 else 0.0
        rows.append((max(err / (ENTRY_BOUND * mx + 1e-4 * G), l2t / 1e-2), err, cerr, mx, n))
        ga.append(g.double().reshape(-1)); gt.append(t.reshape(-1)); gc.append(c.reshape(-1))
    rows.sort(reverse=True)
    ga, gt, gc = torch.cat(ga), torch.cat(gt), torch.cat(gc)
    l2, l2c = float((ga - gt).norm() / gt.norm()), float((gc - gt).norm() / gt.norm())
    cos = float((ga * gt).sum() / (ga.norm() * gt.norm()))
    print("%s: gradient vs fp64 oracle: HIP rel. L2 %.2e (torch-CPU fp32: %.2e), cos %.7f, G %.2e" % (tag, l2, l2c, cos, G))
    for r in rows[:6]:
        print("   %.2f of bound: max err %.2e (cpu32 %.2e), max|g| %.2e  %s" % r)
    assert rows[0][0] < 1.0, "%s: gradient of %s exceeds its bound by a factor %.2f" % (tag, rows[0][4], rows[0][0])
    # global: within 2e-3 / cos 0.99999 — or, where the fp32 torch oracle itself is that far from the exact gradient (resenc with all
    # five levels weighted: torch-CPU 3.3e-3, HIP 5.0e-3), within 1.6x of what the reference's own arithmetic achieves
    cosc = float((gc * gt).sum() / (gc.norm() * gt.norm()))
    assert l2 < max(2e-3, 1.6 * l2c) and (1.0 - cos) < max(1e-5, 4.0 * (1.0 - cosc)), (tag, l2, l2c, cos, cosc)
    return rows[0]


def figures(grads, o32, o64):
    """(HIP rel. L2, fp32-oracle rel. L2, cos, worst tensor as a fraction of its bound, its name) — what compare() judges, as numbers"""
    sd32, sd64 = o32[0], o64[0]
    G = max(float(v.grad.abs().max()) for v in sd64.values() if v.grad is not None)
    ga, gt, gc, worst = [], [], [], (0.0, '')
    for n, g in grads.items():
        t = sd64[n].grad
        if t is None:
            continue
        err, mx = float((g.double() - t).abs().max()), float(t.abs().max())
        l2t = float((g.double() - t).norm() / t.norm()) if float(t.norm()) > 1e-3 * G * t.numel() ** 0.5 else 0.0
        worst = max(worst, (max(err / (ENTRY_BOUND * mx + 1e-4 * G), l2t / 1e-2), n))
        ga.append(g.double().reshape(-1)); gt.append(t.reshape(-1)); gc.append(sd32[n].grad.double().reshape(-1))
    ga, gt, gc = torch.cat(ga), torch.cat(gt), torch.cat(gc)
    return (float((ga - gt).norm() / gt.norm()), float((gc - gt).norm() / gt.norm()), float((ga * gt).sum() / (ga.norm() * gt.norm())),
            worst[0], worst[1])


# ---- branches -----------------------------------------------------------------------------------------------------------------------
BRANCHES = {
    'input:cin1': "Engine.forward: NCDHW with one channel is reshaped",
    'input:cin>1': "Engine.forward: ncdhw_to_ndhwc into the x.ndhwc buffer",
    'fwd:conv': "ConvNormOp.forward on conv3d_fwd",
    'fwd:head': "ConvNormOp.forward of a head on pointwise_fwd",
    'fwd:pw_strided': "ConvNormOp.forward of a strided 1x1x1 skip projection on pointwise_fwd",
    'bwdd:pointwise:acc0': "backward-data of a head on pointwise_fwd, first writer",
    'bwdd:pointwise:acc1': "the same, accumulating",
    'bwdd:pw_strided:acc': "scatter backward-data of a skip projection onto a gradient another consumer wrote",
    'bwdd:pw_strided:zero': "the same as FIRST writer: zero_() of the destination, then scatter",
    'bwdd:strided:acc1': "one-launch strided backward-data, accumulating",
    'bwdd:parity:acc1': "parity-class backward-data (conv3d_fwd with strided placement), accumulating",
    'bwdd:parity:classes<full': "parity classes with fewer classes than input parities (a kernel extent of 1 under stride 2)",
    'bwdd:stride1:acc0': "stride-1 backward-data, first writer",
    'bwdd:stride1:acc1': "stride-1 backward-data, accumulating (the conv1 of an identity residual block)",
    'bwdd:stride1:stats': "stride-1 backward-data that also emits the next norm backward's first pass",
    'bwdd:stride1:two-dest': "backward-data of a concat conv: two destinations split at csplit",
    'bwdd:none': "ConvNormOp.backward of the first layer: no backward-data",
    'norm-bwd:plain': "inorm_lrelu_bwd with its own first pass",
    'norm-bwd:part': "inorm_lrelu_bwd fed the partial sums of the last writer of its gradient",
    'bias:channel_sum': "bias gradient of a bare conv (generic head) through channel_sum",
    'tconv:first-writer': "TConvOp.backward with src.grad_init false",
    'resadd:stats': "ResAddOp.backward on mt_lrelu_bwd_stats",
    'resadd:plain': "ResAddOp.backward on mt_lrelu_bwd",
    'resadd:shared': "ResAddOp.backward: the residual's gradient IS the masked buffer",
    'head:fused': "HeadOp.backward on mt_head_bwd",
    'head:generic': "HeadOp.backward on the generic pointwise + tiled pair",
    'head:done1': "mt_head_bwd produced dbias",
    'head:done0': "mt_head_bwd left dbias to the caller (32 input channels)",
    'head:done0:channel_sum': "... and the head has a bias: channel_sum after the fused launch",
    'head:first-writer': "mt_head_bwd writes dX (the full-resolution head)",
    'head:accumulate': "mt_head_bwd accumulates into dX (the transposed conv above wrote first)",
    'head:skipped': "a head whose dlogits is None neither runs nor counts in `pending`",
    'materialise': "_MaterialiseOp forward and backward (the residual encoder's stem)",
    'pack:main-only': "Engine._pack: one program on the main stream",
    'pack:late': "Engine._pack: the backward-only packings on the side stream",
    'pack:mid': "Engine._pack: the deep layers' forward packings on the side stream (more than 2 MB of packed weights)",
    'heads:final-only-grad': "all_heads=False with gradients (do_ds off in train mode)",
    'heads:skip-final': "_skip_final: forward_to_final_head",
    'fuse:0': "fuse_norm_bwd 0", 'fuse:1': "fuse_norm_bwd 1", 'fuse:2': "fuse_norm_bwd 2", 'fuse:3': "fuse_norm_bwd 3",
    'streams:0': "bwdw_streams 0", 'streams:1': "bwdw_streams 1", 'streams:2': "bwdw_streams 2",
    'io:native': "Engine.io (False, False) with 16-bit operands", 'io:cast-in': "Engine.io (True, False)",
    'io:cast-out': "Engine.io (False, True)", 'io:cast-both': "Engine.io (True, True)",
}

UNREACHABLE = {
    'bwdd:strided:acc0': "the source of a strided conv is a skip (plain U-Net: the decoder's concat conv comes later in forward, so it "
                         "writes the gradient first) or the input of a residual block whose skip projection ran backward before conv1",
    'bwdd:parity:acc0': "the same sources as the one-launch strided form",
    'bwdd:parity:zero': "`len(cls) < full and not acc`: needs acc false, which the line above rules out (p-k1-stride2 has 4 of 8 classes "
                        "and runs accumulating)",
    'tconv:accumulate': "a transposed conv comes after the head of the level below in the op list, so in backward it is the first writer "
                        "of its source's gradient; the head accumulates",
    'resadd:add_': "the residual (block input, or the skip projection's output) always has the shape of the block output, so "
                   "Engine._plan shares the buffer",
    'resadd:copy_': "as resadd:add_: with the buffer always shared neither the add_ nor the copy_ of ResAddOp.backward can run",
    'fwd:pw_strided:refused': "_pw_strided_geom with an input that is no multiple of the stride: the decoder's concat then has no matching "
                              "shape (and SegmentationNetwork requires divisibility)",
    'bwdd:pointwise:strided': "NotImplementedError in ConvNormOp.backward: no builder makes a strided head",
}


# ---- configurations -----------------------------------------------------------------------------------------------------------------
P2 = ((2, 2, 2), (2, 2, 2))
_COMMON_PLAIN = ['fwd:conv', 'fwd:head', 'bwdd:strided:acc1', 'bwdd:stride1:acc0', 'bwdd:stride1:two-dest', 'bwdd:none', 'norm-bwd:plain',
                 'tconv:first-writer', 'head:fused', 'head:done1', 'head:first-writer', 'head:accumulate', 'pack:late', 'streams:1']
_COMMON_RES = ['fwd:conv', 'fwd:head', 'fwd:pw_strided', 'bwdd:pw_strided:acc', 'bwdd:strided:acc1', 'bwdd:stride1:acc0', 'bwdd:stride1:acc1',
               'bwdd:stride1:two-dest', 'bwdd:none', 'norm-bwd:plain', 'tconv:first-writer', 'resadd:plain', 'resadd:shared', 'head:fused',
               'head:done1', 'head:first-writer', 'head:accumulate', 'materialise', 'pack:late', 'streams:1']


def _plain(name, expects=(), drop=(), **kw):
    c = dict(name=name, arch='plain', in_ch=1, base=8, nc=3, pools=P2, kernels=None, shape=(8, 16, 16), B=2, loss='softmax', weights='all',
             ds=True, loss_outputs=None, opts={}, wino=False, streams=None, fuse=None, precision='fp32', seed=5)
    c.update(kw)
    c['expects'] = sorted((set(_COMMON_PLAIN) | {'input:cin1' if c['in_ch'] == 1 else 'input:cin>1'} | set(expects)) - set(drop))
    return c


def _res(name, expects=(), drop=(), **kw):
    c = dict(name=name, arch='resenc', in_ch=1, base=8, nc=3, pools=RESENC_POOLS, kernels=RESENC_KERNELS, blocks=RESENC_BLOCKS, max_features=24,
             shape=(8, 32, 32), B=2, loss='softmax', weights='all', ds=True, loss_outputs=None, opts={}, wino=False, streams=None, fuse=None,
             precision='fp32', seed=5)
    c.update(kw)
    c['expects'] = sorted((set(_COMMON_RES) | {'input:cin1' if c['in_ch'] == 1 else 'input:cin>1'} | set(expects)) - set(drop))
    return c


_B10 = dict(base=10)
_ANISO = dict(pools=((1, 2, 2), (2, 2, 2), (2, 2, 2)), kernels=[[1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]], shape=(4, 32, 16))
_GENERIC_HEAD = dict(expects=['head:generic', 'bwdd:pointwise:acc0', 'bwdd:pointwise:acc1'], drop=['head:fused', 'head:done1', 'head:first-writer',
                                                                                                    'head:accumulate'])
_STREAMS0 = dict(streams=0, expects=['streams:0', 'pack:main-only'], drop=['streams:1', 'pack:late'])
_MIXED = dict(precision='bf16')

CONFIGS = [
    _plain('p-base'),
    _plain('p-base/W', wino=True),
    _plain('p-cin2', in_ch=2, B=1), _plain('p-cin3', in_ch=3, B=1), _plain('p-cin4', in_ch=4, B=1),
    _plain('p-B1', B=1), _plain('p-B3', B=3),
    _plain('p-aniso', **_ANISO), _plain('p-aniso/W', wino=True, **_ANISO),
    _plain('p-mixed-stride', pools=((2, 2, 1), (2, 1, 2)), kernels=[[3, 3, 1], [3, 3, 3], [3, 1, 3]], shape=(8, 8, 8),
           expects=['bwdd:parity:acc1'], drop=['bwdd:strided:acc1']),
    # the one-launch strided kernel refuses a 1x3x3 kernel (it takes 3x3x3, pad 1, stride (1|2, 2, 2)): the parity classes take it,
    # 4 classes for 8 input parities, accumulating onto the gradient the decoder wrote (see UNREACHABLE['bwdd:parity:zero'])
    _plain('p-k1-stride2', kernels=[[3, 3, 3], [1, 3, 3], [3, 3, 3]], expects=['bwdd:parity:acc1', 'bwdd:parity:classes<full']),
    _plain('p-nobias', opts=dict(internal_conv_bias=False)),
    _plain('p-headbias', opts=dict(seg_output_use_bias=True)),
    _plain('p-nc65', nc=65, loss='softmax-torch', **_GENERIC_HEAD),
    _plain('p-nc65-headbias', nc=65, loss='softmax-torch', opts=dict(seg_output_use_bias=True), expects=_GENERIC_HEAD['expects'] + ['bias:channel_sum'],
           drop=_GENERIC_HEAD['drop']),
    _plain('p-base72', base=72, pools=((2, 2, 2),), shape=(4, 8, 8), expects=_GENERIC_HEAD['expects'] + ['pack:mid'],
           drop=_GENERIC_HEAD['drop'] + ['bwdd:pointwise:acc1']),
    # base 32 capped at 48: the full-resolution head has 32 input channels (mt_head_bwd, its narrow form: dbias done), the lower one 48
    # (above mt_head_bwd's 32: the generic pair, accumulating)
    _plain('p-cap', base=32, opts=dict(max_num_features=48), expects=['head:generic', 'bwdd:pointwise:acc1'], drop=['head:accumulate']),
    # six classes: past the narrow form (Cout <= 4), the tiled mt_head_bwd at exactly 32 input channels has no spare MFMA row for dbias
    _plain('p-cap-headbias', base=32, nc=6, opts=dict(max_num_features=48, seg_output_use_bias=True),
           expects=['head:done0', 'head:done0:channel_sum', 'head:generic', 'bwdd:pointwise:acc1', 'bias:channel_sum'],
           drop=['head:done1', 'head:accumulate']),
    _plain('p-base10', **_B10), _plain('p-base10/W', wino=True, **_B10),
    _plain('p-base30', base=30, pools=((2, 2, 2),), drop=['head:accumulate']),
    _plain('p-base30/W', base=30, pools=((2, 2, 2),), wino=True, drop=['head:accumulate']),
    _plain('p-ds-off', ds=False, expects=['heads:final-only-grad', 'head:skipped'], drop=['head:accumulate']),
    # seeds: with seed 5 a voxel of these two sits within fp32 rounding of a LeakyReLU kink and the fp32 ORACLE misses compare() (1.3 and
    # 0.6 of the per-tensor bound against 0.003 elsewhere); 9 and 7 keep the reference three orders inside like every other case
    _plain('p-partial-loss', pools=((2, 2, 2),) * 3, loss_outputs=(0, 2), seed=9),
    _plain('p-zero-weight', weights='ds'),
    _plain('p-multitalent', nc=47, loss='multitalent'),
    _plain('p-streams0', wino=True, **_B10, **_STREAMS0),
    _plain('p-streams2', wino=True, streams=2, expects=['streams:2'], drop=['streams:1'], **_B10),
    _plain('p-fuse0', wino=True, fuse=0, expects=['fuse:0'], **_B10),
    _plain('p-fuse1', wino=True, fuse=1, expects=['fuse:1', 'bwdd:stride1:stats', 'norm-bwd:part'], **_B10),
    _plain('p-fuse2', wino=True, fuse=2, expects=['fuse:2', 'bwdd:stride1:stats', 'norm-bwd:part'], **_B10),
    _plain('p-fuse3', wino=True, fuse=3, expects=['fuse:3'], **_B10),
    _res('r-base', nc=47, loss='multitalent'),
    _res('r-base/W', nc=47, loss='multitalent', wino=True),
    _res('r-blocks-1111', blocks=[1, 1, 1, 1]),
    _res('r-blocks-1232', blocks=[1, 2, 3, 2], seed=7),
    _res('r-pool0-222', pools=[[2, 2, 2], [2, 2, 2], [2, 2, 2]], kernels=[[3, 3, 3]] * 3, blocks=[1, 2, 2], shape=(8, 16, 16),
         expects=['bwdd:pw_strided:zero']),
    _res('r-cin2', in_ch=2),
    _res('r-aniso', pools=[[1, 1, 1], [1, 2, 2], [2, 2, 2]], kernels=[[1, 3, 3], [3, 3, 3], [3, 3, 3]], blocks=[1, 2, 2], shape=(4, 16, 16)),
    _res('r-streams0', wino=True, **_STREAMS0),
    _res('r-fuse0', wino=True, fuse=0, expects=['fuse:0']),
    _res('r-fuse1', wino=True, fuse=1, expects=['fuse:1', 'resadd:stats', 'norm-bwd:part'], drop=['resadd:plain']),
    _res('r-fuse2', wino=True, fuse=2, expects=['fuse:2']),
    _res('r-fuse3', wino=True, fuse=3, expects=['fuse:3', 'resadd:stats', 'norm-bwd:part'], drop=['resadd:plain']),
    _plain('p-base10/bf16', expects=['io:native', 'io:cast-in', 'io:cast-both', 'fuse:3'], **_B10, **_MIXED),
    _plain('p-aniso/bf16', expects=['io:native', 'io:cast-in', 'io:cast-out', 'io:cast-both'], **_ANISO, **_MIXED),
    _res('r-base/bf16', nc=47, loss='multitalent', precision='bf16',
         expects=['io:native', 'io:cast-both', 'resadd:stats', 'norm-bwd:part', 'fuse:3'], drop=['resadd:plain']),
]
CONFIG = {c['name']: c for c in CONFIGS}


# ---- sequences ----------------------------------------------------------------------------------------------------------------------
# yardstick 'fresh': the same network built again from the same seed and taken to the same final state directly, torch.equal on logits
# and every gradient; 'fresh~2e-5': within 2e-5 of the tensor's largest entry (settings that legitimately reorder sums); 'oracle':
# compare() against the fp64 oracle taken through the same steps; 'raises': the refusal is what is pinned
SEQUENCES = [
    dict(name='stock-optimizer', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh', 'oracle'), expects=[],
         steps="two iterations with SGD(momentum 0.99, nesterov) / AdamW and NO mark_params_dirty(); iteration 2 == the loop that marks; vs fp64"),
    dict(name='load-state-dict', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="forward; net.load_state_dict(other); forward == a fresh network loaded with other"),
    dict(name='shape-roundtrip', on=('p-base10', 'r-base'), mixed=True, yardsticks=('fresh',), expects=[],
         steps="train step at (2; 8,16,16), (1; 8,32,16), (3; 16,16,16), the first again; 4th == 1st, each == a fresh engine"),
    dict(name='train-validate-train', on=('p-base10', 'r-base'), mixed=True, yardsticks=('fresh',), expects=['heads:skip-final'],
         steps="train step; eval + no_grad + do_ds off at another batch and shape through net(x) and through predict_3D (tiled, mirrored: "
               "forward_to_final_head); train step == the first; the predictions == a fresh network's"),
    dict(name='nograd-in-train-mode', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="no_grad forward while net.training; then a normal step == a fresh engine's"),
    dict(name='precision-roundtrip', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="fp32, bf16, fp32 on one engine: 1st == 3rd, the middle == a fresh bf16 engine"),
    dict(name='stream-and-fuse-switch', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh', 'fresh~2e-5'), expects=[],
         steps="bwdw_streams 1, 0, 2, 1: identical gradients; fuse_norm_bwd None, 1, 0, 3 within 2e-5; the recorder shows each took effect"),
    dict(name='accumulate-grads', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="two forward/backward pairs without zero_grad: p.grad == float32 sum of the two; p.grad does not alias flat_grad"),
    dict(name='stale-backward', on=('p-base10', 'r-base'), mixed=False, yardsticks=('raises', 'fresh'), expects=[],
         steps="out1 = net(x1); out2 = net(x2); loss(out1).backward() raises RuntimeError (INTEGRATION.md §2 (c)); loss(out2).backward() is right"),
    dict(name='frozen-body', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="requires_grad_(False) on everything but the heads: head gradients == the unfrozen run's, frozen parameters keep grad None"),
    dict(name='rehome', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=[],
         steps="after a step: net.cpu(), net.to(dev), copy.deepcopy(net); the next step of each == a fresh engine's; grad_of serves the copy"),
    dict(name='ds-toggle', on=('p-base10', 'r-base'), mixed=False, yardsticks=('fresh',), expects=['heads:final-only-grad'],
         steps="deep supervision on, off, on in train mode on one engine; each == a fresh engine in that mode"),
]


# ---- cases and the oracle -----------------------------------------------------------------------------------------------------------
def build_net(cfg):
    """-> (net, forward(sd, x, deep_supervision) of the oracle)"""
    if cfg['arch'] == 'plain':
        net, pools, kernels = build_plain(cfg['nc'], base=cfg['base'], pools=cfg['pools'], kernels=cfg['kernels'], in_ch=cfg['in_ch'], **cfg['opts'])
        fwd = lambda sd, x, ds=True: R.generic_unet_forward(sd, x, pools, kernels, deep_supervision=ds)
    else:
        net, pools, kernels, blocks = build_resenc(cfg['nc'], base=cfg['base'], blocks=cfg['blocks'], pools=cfg['pools'], kernels=cfg['kernels'],
                                                   in_ch=cfg['in_ch'], max_features=cfg['max_features'])
        fwd = lambda sd, x, ds=True: R.fabians_unet_forward(sd, x, pools, kernels, blocks, deep_supervision=ds)
    return net, fwd


def output_scales(cfg):
    """spatial scale of every deep-supervision output, highest resolution first"""
    pools = [list(p) for p in cfg['pools']]
    cum, scales = np.ones(3), []
    if cfg['arch'] == 'resenc':          # its first stage pools too; its decoder has one output per stage but the last
        cum = cum / np.array(pools[0])
        pools = pools[1:]
    for p in [None] + pools[:-1]:
        if p is not None:
            cum = cum / np.array(p)
        scales.append([float(c) for c in cum])
    return scales


def loss_weights(cfg):
    n = len(output_scales(cfg))
    if cfg['weights'] == 'ds':            # the trainers': the lowest level has weight zero
        return [float(w) for w in R.ds_loss_weights(n)]
    w = np.array([0.5, 0.3, 0.2, 0.1][:n])
    return [float(v) for v in w / w.sum()]


def valid_regions(cfg, B=None):
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import MultiTalent_valid_regions as V
    names = ['Task003_Liver', 'Task017_AbdominalOrganSegmentation', 'Task046_AbdOrgSegm2']
    return [V[names[b % 3]] for b in range(cfg['B'] if B is None else B)]


def make_case(cfg, shape=None, B=None, seed=None):
    """inputs of one step: x [B, in_ch, *shape], targets per output, weights (+ valid regions) — deterministic in (cfg, shape, B, seed)"""
    shape = tuple(cfg['shape'] if shape is None else shape)
    B = cfg['B'] if B is None else B
    seed = cfg['seed'] if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, cfg['in_ch']) + shape, generator=g)
    targets = make_targets(shape, output_scales(cfg), 23 if cfg['loss'] == 'multitalent' else cfg['nc'], B, seed=seed + 1)
    return dict(x=x, targets=targets, weights=loss_weights(cfg), valid=valid_regions(cfg, B) if cfg['loss'] == 'multitalent' else None)


def selected(cfg, seq):
    """the outputs (targets, weights) the loss of this configuration is taken over"""
    if not cfg['ds']:
        return [seq[0]]
    if cfg['loss_outputs'] is not None:
        return [seq[i] for i in cfg['loss_outputs']]
    return list(seq)


def oracle_loss(cfg, outs, case):
    """loss of the reference on the oracle's outputs -> tuple of values, the first is the one to differentiate"""
    outs = [outs] if torch.is_tensor(outs) else list(outs)
    outs, tg = selected(cfg, outs), selected(cfg, case['targets'])
    w = [1.0] if not cfg['ds'] else selected(cfg, case['weights'])
    if cfg['loss'] == 'multitalent':
        from multitalent_amd.dataset_conversion.Task100_MultiTalent import MultiTalent_region_output_idx_mapping, MultiTalent_regions
        return R.multitalent_loss(outs, tg, case['valid'], MultiTalent_regions, MultiTalent_region_output_idx_mapping, w)
    return (R.multiple_output_loss(outs, tg, w, batch_dice=False),)


def run_oracle(cfg, dtype, sd0, case):
    """oracle/reference_ops.py forward + loss + backward in `dtype` from the weights sd0 -> (sd with .grad, outputs [fp32], losses)"""
    key = base_key(cfg)
    if key not in _FWD:
        _FWD[key] = build_net(cfg)[1]
    fwd = _FWD[key]
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd0.items() if '.all.' not in k}
    out = fwd(sd, case['x'].to(dtype), cfg['ds'])
    ls = oracle_loss(cfg, out, case)
    ls[0].backward()
    out = [out] if torch.is_tensor(out) else list(out)
    return sd, [o.detach().float() for o in out], [l.detach() for l in ls]


_FWD = {}
_ORACLE = {}


def base_key(cfg):
    """configurations that differ only in engine settings share one network, one batch and one oracle result"""
    return repr([(k, cfg[k]) for k in sorted(cfg) if k not in ('name', 'expects', 'wino', 'streams', 'fuse', 'precision')])


def oracle_pair(cfg):
    """(case, sd0, o32, o64), computed once per base configuration and left unchanged"""
    key = base_key(cfg)
    if key not in _ORACLE:
        net, _ = build_net(cfg)
        sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        case = make_case(cfg)
        _ORACLE[key] = (case, sd0, run_oracle(cfg, torch.float32, sd0, case), run_oracle(cfg, torch.float64, sd0, case))
    return _ORACLE[key]


def oracle_train(cfg, dtype, sd0, cases, make_opt):
    """the oracle taken through len(cases) iterations with optimizer steps between them (make_opt(params) -> torch optimizer);
    -> (sd with the LAST iteration's .grad, its outputs, its losses)"""
    key = base_key(cfg)
    if key not in _FWD:
        _FWD[key] = build_net(cfg)[1]
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd0.items() if '.all.' not in k}
    opt = make_opt(list(sd.values()))
    for i, case in enumerate(cases):
        opt.zero_grad(set_to_none=True)
        out = _FWD[key](sd, case['x'].to(dtype), cfg['ds'])
        ls = oracle_loss(cfg, out, case)
        ls[0].backward()
        if i + 1 < len(cases):
            opt.step()
    out = [out] if torch.is_tensor(out) else list(out)
    return sd, [o.detach().float() for o in out], [l.detach() for l in ls]
