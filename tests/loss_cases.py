"""Shared by tests/test_loss_cases_cpu.py and tests/test_loss_kernels_gpu.py (not a test module).

The loss and optimizer kernels (csrc/loss.hip, csrc/optim.hip) on real memory against float64: the case tables of
mt_multitalent_loss_fwd / _bwd, mt_softmax_dice_ce_fwd / _bwd, mt_multitalent_hard_stats, mt_loss_combine, mt_sumsq and mt_sgd_nesterov,
and the references.  The references are plain torch / numpy on the CPU, written from the definitions the header of loss.hip cites
(MultiTalent_Trainer_DDP.py:544-623; dice_loss.py:100-195; crossentropy.py:4-11; nnUNetTrainerV2.py:166-170) and from nothing in the
library; test_loss_cases_cpu.py checks each of them against an independent statement of the same operation.

A case says which kernel it claims (as mt_*_kernel_name prints it) and, for the MultiTalent forward, which body every sample takes inside
mt_loss_fwd_sparse_kernel ('S' sparse: 1 <= popcount(valid[b] & mask(C)) <= 23, 'F' flat).  Operands are views of flat buffers: element
GUARD + off + (b * V + v) * cs + c; everything outside a view holds SENTINEL and must be bit-identical afterwards.

Bounds.  The project's bounds hold for every case: MultiTalent statistics rtol 2e-5, atol 1e-3; MultiTalent gradient rtol 1e-4, atol
1e-5; softmax statistics 1e-4 |ref| + 1e-4; softmax gradient 1e-5 max|gstats|; SGD relerr < 1e-6.  Beside them every statistic meets the
bound of its own accumulation (sum_bound).  All four statistics are sums of non-negative terms, so sum|terms| = ref and
    |got - ref| <= U ((CHAIN + TERM_REL + 1) ref + TERM_ABS n),     U = 2^-24, n = voxels of the sample,
CHAIN = the longest run of fp32 additions of the geometry (a running sum never exceeds ref, so each addition errs by at most U ref), + 1
for the conversion of the float64 sum over blocks to fp32.  CHAIN per body:
  * flat body, nsub = 256 / C threads per channel: ceil(vpb / nsub) additions in a thread, then nsub in the fixed-order sum;
  * sparse body, nsub = 256 / nact: the same with that nsub;
  * strided MultiTalent kernel and the wide softmax kernels (a wave per voxel, 1024 voxels per block): 256 + 4 (+ 6 butterfly levels);
  * register softmax kernels (a thread per voxel): 4 + 6 butterfly levels + 4 waves.
TERM_REL / TERM_ABS, the error of one term before it is added: __expf(-d) errs by (2 + d) U relative (the argument d log2(e) is rounded)
and d exp(-d) < 0.37, the reciprocal instruction and __logf by one ulp of a number in [0.5, 2], the products by U each:
MultiTalent TERM_REL = 4 (max(x, 0) - x y and its sum with the logarithm), TERM_ABS = 8; softmax: the sum of C exponentials adds C U
relative to every probability and C U absolute to log(sum): TERM_REL = C + 6, TERM_ABS = C + 8.
mt_sumsq: a thread adds at most 5 quads (4 products, 4 additions each), a butterfly of 6, 3 additions, the conversion: 64 U relative
(every term is non-negative).  mt_loss_combine: COMBINE_VALUE_MULT U of the float64 value for each of the CE and Dice parts (of their sum
of magnitudes for the loss); COMBINE_GRAD_MULT U of max|g_ref| per level and of |gT| + 2 |gF| = 2 k gscale / den per entry (the size of
the two terms whose difference gT is).  Both multiples are at most four times the worst case measured against float64 on the device.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GUARD = 64
SENTINEL = -7.25
FAKE_BASE = 1 << 20                  # base address of the CPU test's queries (never dereferenced)
LS_VB, LF_KMAX, LF_VMAX, LF_SPARSE_MAX = 1024, 240, 4096, 23

MT_STATS_RTOL, MT_STATS_ATOL = 2e-5, 1e-3
MT_GRAD_RTOL, MT_GRAD_ATOL = 1e-4, 1e-5
SM_STATS_REL, SM_STATS_ABS = 1e-4, 1e-4
SM_GRAD = 1e-5
SGD_RELERR = 1e-6
SUMSQ_MULT = 64
COMBINE_VALUE_MULT, COMBINE_GRAD_MULT = 7, 12       # worst cases measured on an MI355X: 1.99 U and 3.83 U; at most 4x those
MT_TERM_REL, MT_TERM_ABS = 4, 8


def bounds_text():
    return ('U = 2^-24; MultiTalent TERM_REL %d TERM_ABS %d; softmax TERM_REL C + 6 TERM_ABS C + 8; sumsq %d U; combine value %d U, gradient %d U'
            % (MT_TERM_REL, MT_TERM_ABS, SUMSQ_MULT, COMBINE_VALUE_MULT, COMBINE_GRAD_MULT))


def gen(*key):
    """a generator seeded by the key's text (the same in every process)"""
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


def relerr(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def s64(u):
    """an unsigned 64-bit word as the int64 a torch tensor stores"""
    return u - (1 << 64) if u >= (1 << 63) else u


def mask_of(C):
    return (1 << C) - 1 if C < 64 else (1 << 64) - 1


def popcount(x):
    return bin(x).count('1')


def sum_bound(ref, n, chain, term_rel, term_abs):
    return U * ((chain + term_rel + 1) * ref.abs() + term_abs * n)


# ================================================================================================================================
# MultiTalent forward / backward: the launch rules, restated
def lf_nsub(C):
    return 256 // C


def lf_vpb(C):
    return min(LF_KMAX * lf_nsub(C), LF_VMAX)


def mt_fwd_rule(cs, V, C):
    if cs == C:
        return 'mt_loss_fwd_sparse_kernel', lf_vpb(C), -(-V // lf_vpb(C))
    return 'mt_loss_fwd_kernel', LS_VB, -(-V // LS_VB)


def mt_bwd_rule(logits, cs, dlogits, dcs, V, C):
    if cs == C and dcs == C:
        wide = C >= 2 and (V * C) % 4 == 0 and logits % 16 == 0 and dlogits % 16 == 0
        return 'mt_loss_bwd_wide_kernel' if wide else 'mt_loss_bwd_flat_kernel', lf_vpb(C), -(-V // lf_vpb(C))
    return 'mt_loss_bwd_kernel', LS_VB, -(-V // LS_VB)


def mt_body(mask, C):
    return 'S' if 1 <= popcount(mask & mask_of(C)) <= LF_SPARSE_MAX else 'F'


MT_C = [1, 2, 3, 5, 15, 16, 47, 63, 64]
MT_LAYOUTS = {                       # name: (cs - C, dcs - C, base offset in floats)
    'dense': (0, 0, 0),
    'off1': (0, 0, 1),               # both bases 4 bytes into their allocations: the flat backward through the alignment clause
    'strided': (3, 3, 0),
    'dcs': (0, 3, 0),                # contiguous logits, dlogits a slice of a wider buffer
}
MT_LOGITS = ['randn', 'planted', 'scaled']
MT_MASKS = ['few', 'none_all', 'high', 'n23_24', 'all64']
PLANTED = [30.0, -30.0, 88.0, -88.0, 95.0, -95.0, 104.0, -104.0, 0.0, -0.0]
LABEL_PLANTS = [-1, 0, 63, 64, 200, -300] + list(range(64))

MTCase = collections.namedtuple('MTCase', 'id C cs dcs off V masks maskname logits fwd bwd bodies')


def mt_masks(name, C):
    """the valid words of a launch's samples (unsigned)"""
    full, high = mask_of(C), ((1 << 64) - 1) & ~mask_of(C)
    a, b, c = 0, C // 2, C - 1
    few = [1 << b, (1 << a) | (1 << c), (1 << a) | (1 << b) | (1 << c)]           # 1, 2 and 3 regions (fewer where C has no more)
    if name == 'few':
        return few if C > 1 else [1, 0, 1]
    if name == 'none_all':
        return [0, full]
    if name == 'high':               # bits at or above C: they must change nothing
        return [few[0] | high, few[2] | high, high]
    if name == 'n23_24':             # 23 (sparse body) and 24 (flat body) regions in one launch
        if C < 24:
            return [full, 0, 1]
        return [(1 << 23) - 1, ((1 << 24) - 1) << (C - 24), full]
    assert name == 'all64'           # every bit set (C = 63: bit 63 is above C; C = 64: bit 63 is a region), and bit 63 with bit 0
    return [(1 << 64) - 1, (1 << 63) | 1]


def mt_vs(C):
    nsub, vpb = lf_nsub(C), lf_vpb(C)
    vs = [1, nsub - 1, vpb - 1, vpb, vpb + 1] + [2 * vpb + r for r in (1, nsub, nsub + 1, 2 * nsub + 1, 3 * nsub + 1)]
    out = []
    for v in vs:
        if v >= 1 and v not in out:
            out.append(v)
    return out


def _mt_case(C, V, layout, maskname, logits):
    dc, ddc, off = MT_LAYOUTS[layout]
    masks = mt_masks(maskname, C)
    # what the case claims: the kernel of each direction by layout, the body of each sample by its mask
    fwd = 'mt_loss_fwd_kernel' if layout == 'strided' else 'mt_loss_fwd_sparse_kernel'
    if layout in ('strided', 'dcs'):
        bwd = 'mt_loss_bwd_kernel'
    elif layout == 'off1' or C == 1 or (V * C) % 4:
        bwd = 'mt_loss_bwd_flat_kernel'
    else:
        bwd = 'mt_loss_bwd_wide_kernel'
    bodies = '-' * len(masks) if layout == 'strided' else ''.join(mt_body(m, C) for m in masks)
    return MTCase('c%d-v%d-%s-%s-%s' % (C, V, layout, maskname, logits), C, C + dc, C + ddc, off, V, tuple(masks), maskname, logits,
                  fwd, bwd, bodies)


def mt_cases():
    out, seen = [], set()

    def add(c):
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    lay = list(MT_LAYOUTS)
    for ci, C in enumerate(MT_C):
        for i, V in enumerate(mt_vs(C)):
            add(_mt_case(C, V, lay[(i + ci) % 4], MT_MASKS[(i + 2 * ci) % 5], MT_LOGITS[(i + ci) % 3]))
        vpb, nsub = lf_vpb(C), lf_nsub(C)
        # per C: both parities of V * C in the dense layout (wide and flat backward), the alignment clause alone, a partial last block
        # under every layout, 23 next to 24 regions, every bit of the word set
        add(_mt_case(C, vpb, 'dense', 'few', 'planted'))
        add(_mt_case(C, vpb + 1, 'dense', 'few', 'scaled'))
        add(_mt_case(C, 2 * vpb + 4 * nsub, 'off1', 'high', 'planted'))
        add(_mt_case(C, 2 * vpb + 3 * nsub + 1, 'strided', 'n23_24', 'scaled'))
        add(_mt_case(C, 2 * vpb + nsub + 1, 'dcs', 'none_all', 'planted'))
        add(_mt_case(C, 2 * vpb + 4 * nsub, 'dense', 'n23_24', 'randn'))
        add(_mt_case(C, vpb + 4, 'dense', 'all64', 'planted'))
        add(_mt_case(C, 5, 'dense', 'high', 'scaled'))                       # V below the thread count of a channel, V * C odd or not
        for j, r in enumerate((nsub + 1, 2 * nsub + 1, 3 * nsub + 1)):       # the flat backward's last voxel in each slot of its unroll
            add(_mt_case(C, 2 * vpb + r, 'off1', 'none_all', MT_LOGITS[j]))   # (no region: the flat forward body, whatever C)
    return out


def mt_lut(C):
    g = gen('lut', C)
    words = [int(w) for w in torch.randint(0, 2 ** 62, (C,), generator=g, dtype=torch.int64)]
    for c in range(C):
        if c % 3 == 0:
            words[c] |= (1 << 63) | 1                  # bit 0 and bit 63 set
        elif c % 3 == 1:
            words[c] &= ~1                             # both clear
        else:
            words[c] |= 1 << 63
    return words


def plant_labels(lab, shift):
    """lab [V] int64, overwritten in place: every entry of LABEL_PLANTS once where V allows, else as many as fit"""
    V, n = lab.shape[0], len(LABEL_PLANTS)
    if V >= n:
        for i, p in enumerate(LABEL_PLANTS):
            lab[(i * V) // n] = p
    else:
        for v in range(V):
            lab[v] = LABEL_PLANTS[(v + shift * V) % n]
    return lab


def mt_labels(key, B, V):
    lab = torch.randint(-1, 64, (B, V), generator=gen('labels', key))
    for b in range(B):
        plant_labels(lab[b], b)
    return lab.float()


def mt_logits(key, recipe, B, V, C):
    x = torch.randn((B, V, C), generator=gen('logits', key)) * 2.5
    if recipe != 'randn':
        ch = (torch.arange(C, dtype=torch.float32) + 1) / C if recipe == 'scaled' else torch.ones(C)
        n = len(PLANTED)
        for b in range(B):
            for i, val in enumerate(PLANTED):
                if V >= n:
                    x[b, ((i * V) // n + 1 + b) % V] = val * ch
                elif i < V:
                    x[b, i] = PLANTED[(i + b * V) % n] * ch
    return x


def mt_draw(c):
    """host tensors of a case: x [B, V, C] fp32, labels [B, V] fp32, lut / masks as unsigned words, gstats [B, C, 4]"""
    B = len(c.masks)
    return {'x': mt_logits(c.id, c.logits, B, c.V, c.C), 'labels': mt_labels(c.id, B, c.V), 'lut': mt_lut(c.C), 'masks': list(c.masks),
            'gstats': torch.randn((B, c.C, 4), generator=gen('gstats', c.id))}


def mt_targets(labels, lut):
    """y [B, V, C] float64: the label is one of 0..63 and in the channel's set (MultiTalent_Trainer_DDP.py:582-584 as a 64-bit LUT)"""
    lab = labels.long().numpy()                                   # (int) of the kernels: the labels are whole numbers
    inr = (lab >= 0) & (lab < 64)
    sh = np.clip(lab, 0, 63).astype(np.uint64)
    w = np.array(lut, dtype=np.uint64)
    y = ((w[None, None, :] >> sh[:, :, None]) & np.uint64(1)).astype(np.float64) * inr[:, :, None]
    return torch.from_numpy(y)


def mt_active(masks, C):
    return torch.tensor([[(m >> ch) & 1 for ch in range(C)] for m in masks], dtype=torch.float64)


def mt_reference(x, labels, masks, lut, gstats=None):
    """stats [B, C, 4] = (sum BCEWithLogits, tp, fp, fn) over the voxels for the channels a sample carries, 0 elsewhere; and, with
    gstats, d sum(gstats * stats) / dx in closed form (mtseg.h)"""
    x = x.double()
    y = mt_targets(labels, lut)
    act = mt_active(masks, x.shape[2])[:, None, :]
    sg = 1.0 / (1.0 + torch.exp(-x))
    bce = torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    stats = torch.stack(((bce * act).sum(1), (sg * y * act).sum(1), (sg * (1 - y) * act).sum(1), ((1 - sg) * y * act).sum(1)), -1)
    if gstats is None:
        return stats, None
    g = gstats.double()[:, None]
    d = act * (g[..., 0] * (sg - y) + sg * (1 - sg) * (y * (g[..., 1] - g[..., 3]) + (1 - y) * g[..., 2]))
    return stats, d


def mt_last_slot(c, nsub):
    """the slot u of the four-way unroll that holds the last voxel of the last block, for a body with nsub threads per channel"""
    vpb = lf_vpb(c.C)
    return ((c.V - 1) % vpb // nsub) % 4


def mt_chain(c):
    """the longest fp32 addition chain of a case's forward"""
    if c.fwd == 'mt_loss_fwd_kernel':
        return 256 + 4
    vpb, chain = lf_vpb(c.C), 0
    for m, body in zip(c.masks, c.bodies):
        nsub = 256 // popcount(m & mask_of(c.C)) if body == 'S' else lf_nsub(c.C)
        chain = max(chain, -(-vpb // nsub) + nsub)
    return chain


# ================================================================================================================================
# softmax Dice + CE
SM_C = [2, 3, 4, 5, 8, 9, 16, 17, 33, 64]
SM_V = [1, 255, 256, 1024, 1025, 1365]
SM_LAYOUTS = {'dense': (0, 0), 'strided': (3, 0), 'off1': (0, 1)}          # (cs - C == dcs - C, base offset in floats)
SPREADS = [(100.0, 'min'), (100.0, 'max'), (80.0, 'min'), (80.0, 'max'), (100.0, 'mid'), (80.0, 'mid')]
SMCase = collections.namedtuple('SMCase', 'id C cs off V noclass logits fwd bwd')


def sm_maxc(C):
    return 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 0


def sm_name(C, backward):
    m, d = sm_maxc(C), 'bwd' if backward else 'fwd'
    return 'softmax_loss_%s_kernel<%d>' % (d, m) if m else 'softmax_loss_%s_wide_kernel' % d


SM_INSTANCES = ['softmax_loss_%s_kernel<%d>' % (d, m) for d in ('fwd', 'bwd') for m in (4, 8, 16)] + \
               ['softmax_loss_fwd_wide_kernel', 'softmax_loss_bwd_wide_kernel']


def sm_cases():
    out, count = [], collections.Counter()
    claimed = {2: 4, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 17: 0, 33: 0, 64: 0}           # the table's claim: MAXC per class count
    for C in SM_C:
        m = claimed[C]
        for layout, (dc, off) in SM_LAYOUTS.items():
            k = count[m]
            count[m] += 1
            V = SM_V[k % 6]
            fwd = 'softmax_loss_fwd_kernel<%d>' % m if m else 'softmax_loss_fwd_wide_kernel'
            logits = 'spread' if k % 2 == 0 else 'randn'
            out.append(SMCase('c%d-v%d-%s-%s%s' % (C, V, layout, logits, '-noclass' if k % 3 == 1 else ''), C, C + dc, off, V, k % 3 == 1,
                              logits, fwd, fwd.replace('fwd', 'bwd')))
    return out


def sm_draw(c):
    B, V, C = 2, c.V, c.C
    g = gen('softmax', c.id)
    x = torch.randn((B, V, C), generator=g) * 3.0
    lab = torch.randint(0, C, (B, V), generator=g)
    for b in range(B):
        if V >= C:
            for k in range(C):                                   # every class at least once
                lab[b, (k * V) // C] = k
        if c.noclass and V >= 4:
            lab[b, V - 1], lab[b, V // 2] = -1, C                # "no class": y = 0 everywhere, no CE term
        elif c.noclass:
            lab[b, 0] = C if b else -1
        if c.logits == 'spread':
            for i, (S, where) in enumerate(SPREADS):
                if i >= V:
                    break
                v = (V - 2 - i - b) % V if V > len(SPREADS) + 4 else i
                row = torch.linspace(-S, S, C)[torch.randperm(C, generator=g)]
                x[b, v] = row
                if lab[b, v] >= 0 and lab[b, v] < C:
                    lab[b, v] = int({'min': row.argmin(), 'max': row.argmax(), 'mid': row.abs().argmin()}[where])
    gst = torch.randn((B, C, 4), generator=g)
    return {'x': x, 'labels': lab.float(), 'gstats': gst}


def sm_reference(x, labels, gstats=None):
    """stats [B, C, 4] = (CE sum in slot (b, 0, 0), tp, fp, fn) of softmax(x) against the one-hot labels; a label outside 0..C-1 has a
    zero one-hot row and no CE term.  With gstats: d sum(gstats * stats) / dx by float64 autograd, only slot (b, 0, 0) of the CE column."""
    x = x.double().clone().requires_grad_(gstats is not None)
    B, V, C = x.shape
    lab = labels.long()
    ok = (lab >= 0) & (lab < C)
    y = F.one_hot(lab.clamp(0, C - 1), C).double() * ok[..., None]
    lsm = x - torch.logsumexp(x, 2, keepdim=True)
    p = torch.exp(lsm)
    ce = -(lsm * y).sum((1, 2))
    zero = torch.zeros((B, C - 1), dtype=torch.float64)
    stats = torch.stack([torch.cat([ce[:, None], zero], 1), (p * y).sum(1), (p * (1 - y)).sum(1), ((1 - p) * y).sum(1)], 2)
    if gstats is None:
        return stats.detach(), None
    (stats * gstats.double()).sum().backward()
    return stats.detach(), x.grad


def sm_chain(c):
    return 4 + 6 + 4 if sm_maxc(c.C) else 256 + 4 + 6


# ================================================================================================================================
# mt_multitalent_hard_stats
HS_C, HS_V = [1, 47, 64], [1, 1023, 1024, 1025, 4099]
HS_EPS = 1e-3
HSCase = collections.namedtuple('HSCase', 'id C cs V masks maskname')


def hs_cases():
    out = []
    for ci, C in enumerate(HS_C):
        for wi, dc in enumerate((0, 3)):
            for i, V in enumerate(HS_V):
                name = MT_MASKS[(i + wi + 2 * ci) % 5]
                out.append(HSCase('c%d-cs%d-v%d-%s' % (C, C + dc, V, name), C, C + dc, V, tuple(mt_masks(name, C)), name))
    return out


def hs_draw(c):
    """logits randn * 2.5 with every |x| < HS_EPS pushed out to +-HS_EPS, then +0.0 and -0.0 planted: the hard prediction
    sigmoid(x) > 0.5 is x > 0 for every element (fp32 sigmoid of +-1e-3 is 0.5 +- 2.5e-4, of 0 exactly 0.5: not predicted)"""
    B = len(c.masks)
    x = torch.randn((B, c.V, c.C), generator=gen('hard', c.id)) * 2.5
    small = x.abs() < HS_EPS
    x[small] = torch.where(x[small] < 0, -HS_EPS, HS_EPS)
    for b in range(B):
        if c.V == 1 and b % 2 == 0:
            continue                                            # (one voxel: the even samples keep it)
        x[b, (b + 1) % c.V, 0::2] = 0.0
        x[b, (b + 1) % c.V, 1::2] = -0.0
        if c.V > 8:
            x[b, c.V - 1 - b, 0::2] = -0.0
            x[b, c.V - 1 - b, 1::2] = 0.0
    return {'x': x, 'labels': mt_labels(c.id, B, c.V), 'lut': mt_lut(c.C), 'masks': list(c.masks)}


def hs_left_out(x):
    """voxels the reference x > 0 cannot decide: 0 < |x| < HS_EPS (none, by construction)"""
    return int(((x != 0) & (x.abs() < HS_EPS)).sum())


def hs_reference(x, labels, masks, lut):
    """counts [B, C, 3] int64 = (tp, fp, fn) of x > 0 against the region masks, 0 for the channels a sample does not carry"""
    y = mt_targets(labels, lut).numpy().astype(bool)
    p = (x.numpy() > 0)
    act = mt_active(masks, x.shape[2]).numpy().astype(np.int64)
    tp = (p & y).sum(1, dtype=np.int64)
    fp = (p & ~y).sum(1, dtype=np.int64)
    fn = (~p & y).sum(1, dtype=np.int64)
    return np.stack([tp, fp, fn], -1) * act[:, :, None]


# ================================================================================================================================
# mt_loss_combine
CE_ALL, OVER_B = 1, 2
CB_SHAPES = [(1, 1, 2), (3, 1, 47), (3, 2, 42), (1, 3, 86), (5, 4, 47)]              # L * B * C = 2, 141, 252, 258, 940
CB_CONSTS = {'multitalent': (0.0, 0.0, 0.0, 1e-7), 'nnunet': (1e-5, 1e-5, 1e-8, -3e38), 'ddp': (1e-5, 1e-5, 0.0, -3e38)}
CBCase = collections.namedtuple('CBCase', 'id L B C flags c0 stride consts')


def cb_cases():
    out, i = [], 0
    names = list(CB_CONSTS)
    for (L, B, C) in CB_SHAPES:
        for flags in range(4):
            for c0 in (0, 1):
                stride, consts = (4, 3)[(i // 3) % 2], names[i % 3]
                out.append(CBCase('l%db%dc%d-f%d-c0%d-s%d-%s' % (L, B, C, flags, c0, stride, consts), L, B, C, flags, c0, stride, consts))
                i += 1
    return out


def f32(v):
    return float(np.float32(v))


def cb_draw(c):
    """local statistics [L, B, C, 4] fp32: tp / fp / fn log-uniform in 1e3 .. 1.8e6, a BCE / CE sum of that size, a quarter of the (b, c)
    rows exactly zero (regions a sample does not carry), entry 1 with raw just above and entry 2 just below 1e-7 (tp > 0 in both).  With
    stride 3 `dice` is a separate tensor holding twice the local statistics (two ranks with equal statistics) and the scale is 2."""
    g = gen('combine', c.id)
    L, B, C = c.L, c.B, c.C
    k = 1.0 if c.stride == 4 else 2.0
    st = torch.exp(torch.rand((L, B, C, 4), generator=g) * float(np.log(1800.0)) + float(np.log(1e3))).float()
    zero = torch.rand((L, B, C), generator=g) < 0.25
    flat = st.view(-1, 4)
    zf = zero.view(-1)
    zf[:3] = False
    flat[zf] = 0.0
    rows = {'zero': [int(i) for i in torch.nonzero(zf).flatten()], 'above': None, 'below': None}
    if flat.shape[0] > 1:
        flat[1] = torch.tensor([flat[1, 0], 0.4e-7 / k, 0.7e-7 / k, 0.0])          # raw = 1.5e-7
        rows['above'] = 1
    if flat.shape[0] > 2:
        flat[2] = torch.tensor([flat[2, 0], 0.2e-7 / k, 0.0, 0.1e-7 / k])          # raw = 0.5e-7, a numerator above 0
        rows['below'] = 2
    ce_coef = (torch.rand(L, generator=g) + 0.1) / 1e4
    dice_coef = torch.rand(L, generator=g) + 0.1
    return {'stats': st, 'k': k, 'ce_coef': ce_coef, 'dice_coef': dice_coef, 'rows': rows}


def cb_reference(stats, k, ce_coef, dice_coef, flags, c0, consts):
    """(loss, CE part, Dice part) and dLoss/d(local stats) [L, B, C, 4] in float64: the closed form of mtseg.h with the Dice statistics
    k * stats[..., 1:4] (k = 1: the local ones; k = 2: their sum over two ranks, whose all-gather backward hands every rank k times its
    gradient), differentiated by autograd.  Constants as the fp32 numbers the kernel receives."""
    sn, sd, eps, cm = [f32(v) for v in consts]
    s = stats.double().clone().requires_grad_(True)
    cek, dk = ce_coef.double()[:, None], dice_coef.double()[:, None, None]
    bce = s[..., 0] if flags & CE_ALL else s[:, :, :1, 0]
    ce = (cek * bce.sum(2)).sum()
    d = s[..., 1:4]
    # the all-gather of the reference: forward sums the ranks (k * local), backward sums the ranks' identical gradients (k times)
    d = d * k
    if flags & OVER_B:
        d = d.sum(1, keepdim=True)
    T, Fp, N = d[..., 0], d[..., 1], d[..., 2]
    r = (2 * T + sn) / torch.clamp(2 * T + Fp + N + sd + eps, min=cm)
    dc = (dk * r[:, :, c0:]).sum()
    loss = ce - dc
    loss.backward()
    return (float(loss.detach()), float(ce.detach()), float(dc.detach())), s.grad


# ================================================================================================================================
# optimizer
SS_N = [1, 2, 3, 4, 5, 7, 4095, 4096, 4097, 100003, 4194304 + 4099]
SSCase = collections.namedtuple('SSCase', 'id n big')


def ss_cases():
    return [SSCase('n%d' % n, n, None) for n in SS_N] + [SSCase('n4097-1e18', 4097, 1e18), SSCase('n4097-1e20', 4097, 1e20)]


def ss_draw(c):
    x = torch.randn(c.n, generator=gen('sumsq', c.id))
    if c.big:
        x[c.n // 3] = c.big
    return x


def ss_reference(x):
    return float((x.double() ** 2).sum())


SG_HP = (1e-2, 3e-5, 0.99, 12.0)                     # lr, weight decay, momentum, max_norm (nnUNetTrainerV2.py:166-170; clip 12)
SG_STEPS = {1: (None, 'below', 'above'), 255: ('above', 'far', 'inf'), 1025: ('inf', None, 'below'), 100003: ('below', 'above', 'far'),
            2097152 + 1027: ('far', 'inf', None)}
SG_NORM = {'below': 0.5, 'above': 1.001, 'far': 1e4}
SGCase = collections.namedtuple('SGCase', 'id n steps')


def sg_cases():
    return [SGCase('n%d-%s' % (n, '-'.join(str(s) for s in st)), n, st) for n, st in SG_STEPS.items()]


def sg_sumsq(mode):
    """the fp32 squared norm handed to a step (the kernel only reads the number): below, just above, far above max_norm, or inf"""
    if mode is None:
        return None
    return float('inf') if mode == 'inf' else f32((SG_NORM[mode] * SG_HP[3]) ** 2)


def sg_draw(c):
    g = gen('sgd', c.id)
    return {'p': torch.randn(c.n, generator=g), 'buf': torch.randn(c.n, generator=g) * 7.0,           # buf: garbage the first step ignores
            'grads': [torch.randn(c.n, generator=g) * s for s in (0.2, 1e-3, 5.0)]}


def sg_reference(p, buf, g, first, sumsq, hp=SG_HP):
    """one step in float64 on the stored values: g' = coef g + wd p; buf = g' (first) or mom buf + g'; p -= lr (g' + mom buf);
    coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) (clip_grad_norm_), 1 without a norm, 0 for an infinite one"""
    lr, wd, mom, mx = [f32(v) for v in hp]
    coef = 1.0
    if sumsq is not None:
        coef = min(1.0, mx / (float(np.sqrt(np.float64(sumsq))) + f32(1e-6)))
    p, buf, g = p.double(), buf.double(), g.double()
    gv = g * coef + wd * p
    b = gv if first else mom * buf + gv
    return p - lr * (gv + mom * b), b
