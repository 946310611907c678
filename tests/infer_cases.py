"""Shared by tests/test_infer_cases_cpu.py and tests/test_infer_kernels_gpu.py (not a test module).

The prediction path on real memory against float64: the case lists of the fused inference heads (csrc/head_infer.hip: two kernels,
four instances each), of mt_flip_accumulate, mt_extract_tiles, mt_tile_accumulate, mt_normalize_threshold and mt_resample_classify
(csrc/infer.hip), and the references.  The references are plain numpy / torch on the CPU, written from the operations' definitions
(neural_network.py:384-417,531-591; preprocessing.py:109-197) and from nothing in the library; test_infer_cases_cpu.py checks each of
them against an independent statement of the same operation.

Bounds.  Fused heads and mt_flip_accumulate: relerr = max|got - ref| / max|ref| < 1e-5, the project's bound for these kernels
(test_fused_inference_heads_dword_source).  mt_tile_accumulate: one multiply and one add, each rounded once or fused: 2^-22 max|ref|.
mt_normalize_threshold: one division, one fp32 ulp of the float64 quotient.  mt_resample_classify: seven fp32 lerps of values in
[0, 1] err by less than 1e-6; voxels whose float64 value lies within RS_MARGIN = 1e-5 of a decision are left out (at most RS_MAX_OUT of
a case), every other voxel is exact.
"""
import collections
import itertools

import numpy as np
import torch
import torch.nn.functional as F

MT_F32, MT_BF16, MT_F16 = 0, 1, 2
HEAD_BOUND = 1e-5
GUARD = 64
SENTINEL = -7.25
_BASE = 0x7f0000000000            # fake device addresses of the CPU test (256-byte aligned, never dereferenced)


def relerr(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def gen(*key):
    """a generator seeded by the key's text (the same in every process)"""
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


# ---- the un-flip, as index arithmetic: out[.., d, h, w] = t[.., fd(d), fh(h), fw(w)], f(i) = size - 1 - i where the code's bit is set
def unflip(t, code):
    """code: bit 0 D, bit 1 H, bit 2 W, over the LAST three axes of t"""
    D, H, W = t.shape[-3:]
    di = torch.arange(D - 1, -1, -1) if code & 1 else torch.arange(D)
    hi = torch.arange(H - 1, -1, -1) if code & 2 else torch.arange(H)
    wi = torch.arange(W - 1, -1, -1) if code & 4 else torch.arange(W)
    return t[..., di[:, None, None], hi[None, :, None], wi[None, None, :]]


def bits(code):
    return (bool(code & 1), bool(code & 2), bool(code & 4))


def nonlin_ref(logits, nonlin, dim):
    return logits if nonlin == 0 else (torch.sigmoid(logits) if nonlin == 1 else torch.softmax(logits, dim))


# ================================================================================================================================
# fused heads
INSTANCES = ['d1', 'p2', 'f16', 'bf16']              # <1, MT_F32> | <2, MT_F32> | <2, MT_F16> | <2, MT_BF16>
INST_ARGS = {'d1': (1, MT_F32), 'p2': (2, MT_F32), 'f16': (2, MT_F16), 'bf16': (2, MT_BF16)}
INST_DT = {'d1': torch.float32, 'p2': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
CC = [(30, 47), (32, 3), (16, 32), (20, 33), (8, 64), (48, 1)]
VOX = [(3, 5, 7), (2, 4, 16), (3, 1, 43), (3, 5, 77)]               # 105 | exactly 128 | 129 | 1155: ten workgroups, a partial last one
NSAMP = [1, 2, 4, 8]
WEIGHTS = [1.0, 0.125, 0.3]
SLOPES = [0.01, 1.5]
ORIGINS = ['zero', 'interior', 'corner']
SPREAD, SPREAD_WIDE = 80.0, 100.0          # (exp(80) is finite in fp32: only the wider spread overflows a softmax that subtracts no maximum)

HeadCase = collections.namedtuple('HeadCase', 'id inst cin cout shape cs c0 ns sample0 flips aff slope bias nonlin spread '
                                              'fweights fsamples fflips gauss nb origin')


def _layout(inst, cin, i):
    """(channel stride, first channel) of the source slice inside its wider buffer"""
    if inst == 'd1':
        return [((cin + 2) | 1, 1), (cin + 4, 1), ((cin + 2) | 1, 2)][i % 3]     # odd stride and base 4 mod 8 | base 4 mod 8 | odd stride
    if inst == 'p2':
        return (cin + 4, 2)
    return [(cin + 4, 2), (cin + 8, 8)][i % 2]                                   # base 4 bytes / 16 bytes into a 16-byte line


def head_cases():
    out = []
    for a, inst in enumerate(INSTANCES):
        rows = [(i, CC[i], None) for i in range(6)]
        if inst in ('f16', 'bf16'):
            # Cin 30 at a channel stride of 30, and at stride 34 from a base 4 bytes past 16-byte alignment: the 16-byte load of a
            # lane is then only dword-aligned, and the last lanes' loads run into the next voxel / past the sample
            rows += [(6, (30, 47), (30, 0)), (7, (30, 47), (34, 2))]
        rows += [(8, (20, 33), None)]                  # softmax over logits spread over +-SPREAD_WIDE (set below)
        for i, (cin, cout), lay in rows:
            cs, c0 = lay if lay is not None else _layout(inst, cin, i)
            ns = NSAMP[(i + 2 * a) % 4]
            nonlin = (i + a) % 3
            out.append(HeadCase(
                id='%s-%dto%d-v%d-n%d-i%d' % (inst, cin, cout, int(np.prod(VOX[(i + a) % 4])), ns, i), inst=inst, cin=cin, cout=cout,
                shape=VOX[(i + a) % 4], cs=cs, c0=c0, ns=ns, sample0=(i // 2 + a) % 2, flips=tuple((3 * k + i + a) % 8 for k in range(ns)),
                aff=(i + a) % 3 != 0, slope=SLOPES[(i + a) % 2], bias=(i // 2 + a) % 2 == 0, nonlin=nonlin, spread=SPREAD if (i >= 3 and nonlin != 0) else 0.0,
                fweights=(WEIGHTS[(i + 2 * a) % 3], WEIGHTS[(i + 2 * a + 1) % 3]), fsamples=((i // 2 + a) % 2 + ns - 1, (i // 2 + a) % 2),
                fflips=((i + 3 * a) % 8, (i + 3 * a + 5) % 8), gauss=(i + a) % 2 == 0, nb=(i % 3 + a) % 2 == 0, origin=ORIGINS[(i + a) % 3]))
            if i == 8:
                out[-1] = out[-1]._replace(id=out[-1].id + '-wide', nonlin=2, spread=SPREAD_WIDE)
    return out


def head_N(c):
    return c.sample0 + c.ns


def head_name(c, mirror):
    return 'head_%s_accumulate_kernel<%d, %d>' % (('mirror' if mirror else 'flip',) + INST_ARGS[c.inst])


def head_agg_geometry(c):
    """(aggregate dims, tile origin)"""
    D, H, W = c.shape
    if c.origin == 'zero':
        return (D + 2, H + 3, W + 1), (0, 0, 0)
    if c.origin == 'interior':
        return (D + 3, H + 3, W + 4), (1, 2, 2)
    return (D + 2, H + 1, W + 3), (2, 1, 3)             # x0 + Db == aX, and likewise for y and z


def head_draw(c):
    """everything a case needs, on the host.  x is already rounded to the storage type (the kernels widen exactly)."""
    g = gen('head', c.id)
    N, (D, H, W) = head_N(c), c.shape
    dt = INST_DT[c.inst]
    x = torch.randn((N, D, H, W, c.cin), generator=g).to(dt)
    d = {'x': x}
    if c.aff:
        d['scale'] = torch.rand((N, c.cin), generator=g) + 0.5                 # differ between samples
        d['shift'] = torch.randn((N, c.cin), generator=g) * 0.5
    w = torch.randn((c.cout, c.cin, 1, 1, 1), generator=g) / np.sqrt(c.cin)
    b = torch.randn(c.cout, generator=g) if c.bias else None
    if c.spread:                                                               # logits spread over +-SPREAD
        lg = head_logits(x, d.get('scale'), d.get('shift'), c.slope, w, b)
        k = c.spread / float(lg.flatten()[lg.abs().argmax()])                  # signed: the extreme logit becomes +spread
        w = (w.double() * k).float()
        b = (b.double() * k).float() if b is not None else None
    d['w'], d['b'] = w, b
    d['gauss'] = torch.rand((D, H, W), generator=g) + 0.01 if c.gauss else None
    adims, _ = head_agg_geometry(c)
    d['agg0'] = torch.randn((c.cout,) + adims, generator=g)                     # prior contents
    d['nb0'] = torch.rand(adims, generator=g) * 3
    return d


def head_buffer(c, d):
    """the wider source buffer [N, D, H, W, cs]: the slice holds x, its neighbours the largest finite value the kernels may meet"""
    dt = INST_DT[c.inst]
    buf = torch.full(tuple(d['x'].shape[:4]) + (c.cs,), 65504.0 if dt == torch.float16 else 1e30).to(dt)
    buf[..., c.c0:c.c0 + c.cin] = d['x']
    return buf


def head_logits(x, scale, shift, slope, w, b):
    """[N, Cout, D, H, W] float64 = conv1x1x1(lrelu(x * scale + shift)) + b (F.conv3d in float64 on the CPU)"""
    a = x.double().permute(0, 4, 1, 2, 3)
    if scale is not None:
        t = a * scale.double()[:, :, None, None, None] + shift.double()[:, :, None, None, None]
        a = torch.where(t > 0, t, t * slope)
    return F.conv3d(a, w.double(), b.double() if b is not None else None)


def head_pred(c, d):
    return nonlin_ref(head_logits(d['x'], d.get('scale'), d.get('shift'), c.slope, d['w'], d['b']), c.nonlin, 1)


def head_flip_ref(c, pred):
    """(acc after the `first` launch, acc after the accumulating launch) [Cout, D, H, W] float64"""
    one = c.fweights[0] * unflip(pred[c.fsamples[0]], c.fflips[0])
    return one, one + c.fweights[1] * unflip(pred[c.fsamples[1]], c.fflips[1])


def head_mirror_weight(c):
    return 1.0 / c.ns                                   # the mean over the mirror combinations


def head_mirror_ref(c, d, pred):
    """(agg float64, nb float32 — one fp32 add per voxel, exact) after the launch on the prior contents"""
    adims, o = head_agg_geometry(c)
    s = sum(unflip(pred[c.sample0 + k], c.flips[k]) for k in range(c.ns))
    g = d['gauss'].double() if d['gauss'] is not None else torch.ones(c.shape, dtype=torch.float64)
    sl = tuple(slice(o[i], o[i] + c.shape[i]) for i in range(3))
    agg = d['agg0'].double().clone()
    agg[(slice(None),) + sl] += g * head_mirror_weight(c) * s
    nb = d['nb0'].clone()
    nb[sl] = nb[sl] + (d['gauss'] if d['gauss'] is not None else torch.ones(c.shape))
    return agg, nb


def head_problem(c, base=_BASE, N=None):
    """mt_pointwise_t of a case over a source buffer at `base` (a fake address on the CPU; weights / bias / out left NULL)"""
    from multitalent_amd._lib import mt_pointwise_t
    p = mt_pointwise_t()
    p.src.ptr = base + c.c0 * (4 if INST_ARGS[c.inst][1] == MT_F32 else 2)
    p.src.cs, p.src.C, p.src.dtype = c.cs, c.cin, INST_ARGS[c.inst][1]
    p.src.slope = c.slope
    p.N = head_N(c) if N is None else N
    p.Db, p.Hb, p.Wb = c.shape
    p.Di, p.Hi, p.Wi = c.shape
    p.siD = p.siH = p.siW = p.soD = p.soH = p.soW = 1
    p.Cin, p.Cout = c.cin, c.cout
    p.ocs, p.odtype = c.cout, MT_F32
    return p


# ================================================================================================================================
# mt_flip_accumulate
FA_C = [1, 2, 47, 64, 65, 159]                         # 64: the first size over 64 KB of LDS; 159: the largest that is accepted
FA_W = [1, 7, 256, 257, 300]
FlipAccCase = collections.namedtuple('FlipAccCase', 'id C shape cs c0 code nonlin spread weights')


def flipacc_cases():
    out = []
    for i, (W, fw) in enumerate(itertools.product(FA_W, (0, 1))):
        C = FA_C[i % 6]
        code = ((i // 2) % 2) | (((i // 4) % 2) << 1) | (fw << 2)               # every (D, H) pair with and without the W flip
        nonlin = (i + i // 6) % 3
        out.append(FlipAccCase('C%d-W%d-f%d-nl%d' % (C, W, code, nonlin), C, (2, 3, W), C + 3, 1, code, nonlin, SPREAD if nonlin != 0 and i >= 5 else 0.0,
                               (WEIGHTS[(i + i // 3) % 3], WEIGHTS[(i + i // 3 + 1) % 3])))
    # the largest C and the first C over 64 KB + 1 with the column loop and a W flip
    out.append(FlipAccCase('C159-W300-f7-nl2', 159, (2, 2, 300), 162, 1, 7, 2, SPREAD, (0.125, 0.3)))
    out.append(FlipAccCase('C65-W257-f4-nl0', 65, (3, 2, 257), 68, 1, 4, 0, 0.0, (0.125, 1.0)))
    out.append(FlipAccCase('C47-W7-f3-nl2-wide', 47, (2, 3, 7), 50, 1, 3, 2, SPREAD_WIDE, (1.0, 0.3)))
    return out


def flipacc_draw(c):
    g = gen('flipacc', c.id)
    D, H, W = c.shape
    lg = torch.randn((D, H, W, c.C), generator=g) * 2
    if c.spread:
        lg = lg * (c.spread / float(lg.flatten()[lg.abs().argmax()]))          # signed: the extreme logit becomes +spread
    buf = torch.full((1, D, H, W, c.cs), 1e30)
    buf[0, ..., c.c0:c.c0 + c.C] = lg
    return {'logits': lg, 'buf': buf}


def flipacc_ref(c, d):
    """(after first = 1, after first = 0 on top) [C, D, H, W] float64"""
    pred = unflip(nonlin_ref(d['logits'].double(), c.nonlin, 3).permute(3, 0, 1, 2), c.code)
    return c.weights[0] * pred, c.weights[0] * pred + c.weights[1] * pred


def flipacc_exact(c):
    """nonlin 0, a power-of-two weight, first = 1: one exact multiplication"""
    return c.nonlin == 0 and c.weights[0] in (1.0, 0.125)


# ================================================================================================================================
# mt_extract_tiles: (id, C, volume dims, patch, tiles [((x0, y0, z0), code)])
def extract_cases():
    def tiles(n, vol, patch, key):
        r = np.random.RandomState(key)
        hi = [v - p for v, p in zip(vol, patch)]
        t = [(tuple(int(r.randint(0, h + 1)) for h in hi), int(r.randint(0, 8))) for _ in range(n)]
        t[0] = ((hi[0], hi[1], hi[2]), 7)                                       # the far corner, every axis flipped
        if n > 1:
            t[1] = ((0, 0, 0), 0)
        return t
    return [('t1', 2, (5, 9, 11), (3, 4, 5), tiles(1, (5, 9, 11), (3, 4, 5), 1)),
            ('t9', 3, (7, 9, 13), (3, 4, 5), tiles(9, (7, 9, 13), (3, 4, 5), 2)),
            ('t64', 1, (6, 7, 9), (2, 3, 4), tiles(64, (6, 7, 9), (2, 3, 4), 3)),
            ('t9-hw1221', 2, (4, 40, 41), (3, 33, 37), tiles(9, (4, 40, 41), (3, 33, 37), 4))]     # H*W > 1024: the inner loop iterates


def extract_ref(vol, patch, tiles):
    """torch.flip of the slices (neural_network.py:531-586)"""
    out = []
    for (x0, y0, z0), code in tiles:
        t = vol[:, x0:x0 + patch[0], y0:y0 + patch[1], z0:z0 + patch[2]]
        dims = [1 + i for i in range(3) if code & (1 << i)]
        out.append(torch.flip(t, dims) if dims else t)
    return torch.stack(out)


# ================================================================================================================================
# mt_tile_accumulate
TILE_BOUND = 2.0 ** -22
TileCase = collections.namedtuple('TileCase', 'id C patch adims origin gauss nb')


def tile_cases():
    return [TileCase('c5-zero', 5, (3, 5, 7), (5, 8, 9), (0, 0, 0), True, True),
            TileCase('c5-corner', 5, (3, 5, 7), (5, 8, 9), (2, 3, 2), True, False),
            TileCase('c47-interior-nogauss', 47, (2, 9, 33), (4, 12, 40), (1, 2, 5), False, True),
            TileCase('c1-corner-nogauss-nonb', 1, (4, 4, 65), (4, 6, 65), (0, 2, 0), False, False),
            # 8 x 512 x 520 = 2 129 920 voxels: more than 8192 blocks of 256, the grid-stride loop runs
            TileCase('c1-stride-loop', 1, (8, 512, 520), (9, 512, 521), (1, 0, 1), True, True)]


def tile_draw(c):
    g = gen('tile', c.id)
    return {'acc': torch.randn((c.C,) + c.patch, generator=g), 'gauss': torch.rand(c.patch, generator=g) + 0.01 if c.gauss else None,
            'agg0': torch.randn((c.C,) + c.adims, generator=g), 'nb0': torch.rand(c.adims, generator=g) * 3}


def tile_ref(c, d):
    sl = tuple(slice(o, o + s) for o, s in zip(c.origin, c.patch))
    g = d['gauss'] if d['gauss'] is not None else torch.ones(c.patch)
    agg = d['agg0'].double().clone()
    agg[(slice(None),) + sl] += d['acc'].double() * g.double()
    nb = d['nb0'].clone()
    nb[sl] = nb[sl] + g
    return agg, nb


# ================================================================================================================================
# mt_normalize_threshold
NormCase = collections.namedtuple('NormCase', 'id C V order nb seg')


def norm_cases():
    o5, o47 = [3, 1, 4, 2, 5], [int(v) for v in np.random.RandomState(7).permutation(47) + 1]
    return [NormCase('c1-regions', 1, 777, [9], True, True), NormCase('c1-argmax-nonb', 1, 300, None, False, True),
            NormCase('c5-regions', 5, 1031, o5, True, True), NormCase('c5-argmax', 5, 1031, None, True, True),
            NormCase('c5-regions-nonb', 5, 513, o5, False, True), NormCase('c5-argmax-noseg', 5, 513, None, True, False),
            NormCase('c47-regions', 47, 2049, o47, True, True), NormCase('c47-argmax-nonb', 47, 2049, None, False, True),
            NormCase('c47-regions-noseg', 47, 255, o47, True, False),
            # 16384 x 256 + 77 voxels: the grid-stride loop runs
            NormCase('c1-stride-loop', 1, 16384 * 256 + 77, [3], True, True)]


def norm_draw(c):
    """aggregate and weights with exact ties and exact 0.5 quotients planted"""
    g = gen('norm', c.id)
    nb = torch.rand(c.V, generator=g) * 3 + 0.05 if c.nb else None
    den = nb if nb is not None else torch.ones(c.V)
    agg = torch.rand((c.C, c.V), generator=g) * den
    v = torch.arange(c.V)
    half = v % 11 == 3
    agg[c.C // 2, half] = den[half] * 0.5                      # the quotient is exactly 0.5: not above the threshold
    agg[c.C - 1, v % 13 == 5] = den[v % 13 == 5] * 0.5
    if c.C > 1:
        tie = v % 7 == 2
        top = agg[:, tie].max(0).values * 1.25                 # two equal maxima: argmax takes the first
        agg[1, tie] = top
        agg[c.C - 1, tie] = top
    return {'agg': agg, 'nb': nb}


def decide_ref(probs, order):
    """probs [C, ...] -> labels: regions take the LAST channel above 0.5 (painted in order, neural_network.py:404-412), argmax the first
    maximum"""
    probs = np.asarray(probs)
    if order is None:
        best, seg = probs[0].copy(), np.zeros(probs.shape[1:], np.int64)
        for ch in range(1, probs.shape[0]):
            up = probs[ch] > best
            best, seg = np.where(up, probs[ch], best), np.where(up, ch, seg)
        return seg
    seg = np.zeros(probs.shape[1:], np.int64)
    for ch in range(probs.shape[0]):
        seg = np.where(probs[ch] > 0.5, int(order[ch]), seg)
    return seg


# ================================================================================================================================
# mt_resample_classify
RS_MARGIN, RS_MAX_OUT = 1e-5, 0.01
RsCase = collections.namedtuple('RsCase', 'id C ishape oshape sep order full off')


def resample_cases():
    o3, o5, o47 = [2, 3, 1], [3, 1, 4, 2, 5], [int(v) for v in np.random.RandomState(7).permutation(47) + 1]
    fit = lambda o: tuple(o)
    return [RsCase('up-5x7x9-regions-c5', 5, (5, 7, 9), (9, 16, 11), -1, o5, (12, 18, 14), (2, 1, 3)),
            RsCase('up-5x7x9-argmax-c3-clipD', 3, (5, 7, 9), (9, 16, 11), -1, None, (10, 18, 12), (4, 2, 0)),
            RsCase('sep0-4x9x13-regions-c47-clipH', 47, (4, 9, 13), (9, 5, 29), 0, o47, (9, 6, 30), (0, 3, 1)),
            RsCase('sep1-9x14x16-argmax-c5-clipW', 5, (9, 14, 16), (4, 5, 7), 1, None, (6, 6, 8), (1, 0, 4)),
            RsCase('sep2-4x9x13-regions-c47', 47, (4, 9, 13), (9, 20, 29), 2, o47, (9, 20, 29), (0, 0, 0)),
            RsCase('sep2-4x9x13-argmax-c47-clipall', 47, (4, 9, 13), (9, 20, 29), 2, None, (8, 19, 27), (2, 3, 5)),
            RsCase('identity-regions-c3', 3, (4, 6, 7), (4, 6, 7), -1, o3, (5, 7, 8), (1, 1, 1)),
            RsCase('identity-argmax-c5-sep0', 5, (4, 6, 7), (4, 6, 7), 0, None, fit((4, 6, 7)), (0, 0, 0)),
            RsCase('single-voxel-axes-regions-c5', 5, (1, 6, 1), (4, 9, 5), -1, o5, (5, 9, 6), (1, 0, 1)),
            RsCase('single-voxel-axis-argmax-c3-sep0', 3, (1, 5, 6), (3, 8, 4), 0, None, (3, 8, 4), (0, 0, 0))]


# more than 65536 x 256 output voxels, one channel: the grid-stride loop runs (its reference is computed on the device in float64)
RS_LARGE = RsCase('c1-stride-loop', 1, (4, 9, 13), (260, 260, 250), -1, [6], (260, 261, 250), (0, 1, 0))


def rs_probs(c):
    return torch.rand((c.C,) + c.ishape, generator=gen('rs', c.id))           # uniform random probabilities


def axis_coords(I, O, nearest):
    """(i0, i1, f) float64 per output index: x = (o + 0.5) I / O - 0.5 clamped to [0, I - 1] (skimage resize order 1, mode 'edge' =
    scipy zoom grid_mode); the separate axis samples floor(x + 0.5) (map_coordinates order 0, mode 'nearest')"""
    x = (np.arange(O, dtype=np.float64) + 0.5) * (float(I) / float(O)) - 0.5
    if nearest:
        i = np.clip(np.floor(x + 0.5).astype(np.int64), 0, I - 1)
        return i, i, np.zeros(O)
    xc = np.clip(x, 0.0, float(I - 1))
    i0 = np.floor(xc).astype(np.int64)
    return i0, np.minimum(i0 + 1, I - 1), xc - i0


def resample_values(probs, oshape, sep, xp=np):
    """float64 resampled probabilities [C, OD, OH, OW]; xp = numpy, or torch for tensors on a device (the same gathers)"""
    p = probs.astype(np.float64) if xp is np else probs.double()
    for ax in range(3):
        i0, i1, f = axis_coords(p.shape[1 + ax], oshape[ax], sep == ax)
        if xp is not np:
            i0, i1, f = (torch.as_tensor(t, device=p.device) for t in (i0, i1, f))
        shp = [1, 1, 1, 1]
        shp[1 + ax] = -1
        a = xp.take(p, i0, 1 + ax) if xp is np else p.index_select(1 + ax, i0)
        b = xp.take(p, i1, 1 + ax) if xp is np else p.index_select(1 + ax, i1)
        p = a + f.reshape(shp) * (b - a)
    return p


def resample_excluded(vals, order):
    """voxels within RS_MARGIN of a decision: a value near 0.5 (regions), the two largest near each other (argmax)"""
    if order is not None:
        return (np.abs(vals - 0.5) < RS_MARGIN).any(0)
    if vals.shape[0] < 2:
        return np.zeros(vals.shape[1:], bool)
    srt = np.sort(vals, 0)
    return (srt[-1] - srt[-2]) < RS_MARGIN


def resample_box(c):
    """slices of the full volume that are written, and of the resampled box that lands there (clipped to the volume)"""
    n = [min(o, F_ - b) for o, F_, b in zip(c.oshape, c.full, c.off)]
    return tuple(slice(b, b + k) for b, k in zip(c.off, n)), tuple(slice(0, k) for k in n)
