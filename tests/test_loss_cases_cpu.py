"""The case tables of the loss and optimizer kernels (tests/loss_cases.py) without a GPU: every float64 reference against an independent
statement of the same operation, every case's kernel by name (the three queries are host functions) and by a restatement of the launch
rule, a census of the rule over all channel counts, the geometry each case claims, and the hard-statistics construction."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC

MT_NAMES = {'mt_loss_fwd_kernel', 'mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'mt_loss_bwd_flat_kernel', 'mt_loss_bwd_kernel'}


def _ops():
    from multitalent_amd import ops
    return ops


def _addr(off):
    return LC.FAKE_BASE + 4 * (LC.GUARD + off)


# ---- references ----------------------------------------------------------------------------------------------------------------
def test_multitalent_reference_is_bce_with_logits_and_sigmoid():
    cases = [c for c in LC.mt_cases() if c.V <= 600][:12] + [c for c in LC.mt_cases() if c.logits == 'scaled' and c.C == 47][:2]
    assert len({c.logits for c in cases}) == 3
    for c in cases:
        d = LC.mt_draw(c)
        x = d['x'].double().requires_grad_(True)
        y = torch.zeros_like(x)
        lab = d['labels']
        for ch in range(c.C):                                       # the set of a channel, label value by label value
            for v in range(64):
                if (d['lut'][ch] >> v) & 1:
                    y[:, :, ch] += (lab == v).double()
        act = torch.tensor([[float(bool(m & (1 << ch))) for ch in range(c.C)] for m in c.masks], dtype=torch.float64)[:, None, :]
        bce = F.binary_cross_entropy_with_logits(x, y, reduction='none')
        sg = torch.sigmoid(x)
        want = torch.stack(((bce * act).sum(1), (sg * y * act).sum(1), (sg * (1 - y) * act).sum(1), ((1 - sg) * y * act).sum(1)), -1)
        (want * d['gstats'].double()).sum().backward()
        stats, dx = LC.mt_reference(d['x'], d['labels'], d['masks'], d['lut'], d['gstats'])
        assert torch.allclose(stats, want.detach(), rtol=1e-12, atol=1e-12), c.id
        assert torch.allclose(dx, x.grad, rtol=1e-10, atol=1e-12), c.id
        assert (stats >= 0).all()                                   # sums of non-negative terms: sum|terms| = ref in sum_bound


def test_softmax_reference_is_cross_entropy_and_one_hot_dice():
    for c in LC.sm_cases():
        d = LC.sm_draw(c)
        x = d['x'].double().requires_grad_(True)
        lab = d['labels'].long()
        B, V, Cn = x.shape
        ok = (lab >= 0) & (lab < Cn)
        ce = F.cross_entropy(x.reshape(B * V, Cn), torch.where(ok, lab, torch.full_like(lab, -100)).reshape(-1), ignore_index=-100,
                             reduction='none').reshape(B, V).sum(1)
        p = torch.softmax(x, 2)
        y = torch.zeros_like(p)
        for b in range(B):
            for v in range(V):
                if ok[b, v]:
                    y[b, v, lab[b, v]] = 1.0
        cols = [(p * y).sum(1), (p * (1 - y)).sum(1), ((1 - p) * y).sum(1)]
        g = d['gstats'].double()
        total = (ce * g[:, 0, 0]).sum() + sum((cols[k] * g[:, :, k + 1]).sum() for k in range(3))
        total.backward()
        stats, dx = LC.sm_reference(d['x'], d['labels'], d['gstats'])
        assert torch.allclose(stats[:, 0, 0], ce.detach(), rtol=1e-12, atol=1e-12), c.id
        assert float(stats[:, 1:, 0].abs().max()) == 0.0            # only slot (b, 0, 0) of the CE column
        for k in range(3):
            assert torch.allclose(stats[:, :, k + 1], cols[k].detach(), rtol=1e-12, atol=1e-12), c.id
        assert torch.allclose(dx, x.grad, rtol=1e-9, atol=1e-12), c.id
        assert stats.shape == (B, Cn, 4)


def test_softmax_cases_carry_what_they_claim():
    cases = LC.sm_cases()
    assert len({c.id for c in cases}) == len(cases) == 30
    ops = _ops()
    seen = set()
    for c in cases:
        assert ops.softmax_dice_ce_kernel_name(c.C, False) == c.fwd == LC.sm_name(c.C, False), c.id
        assert ops.softmax_dice_ce_kernel_name(c.C, True) == c.bwd == LC.sm_name(c.C, True), c.id
        seen |= {c.fwd, c.bwd}
    assert seen == set(LC.SM_INSTANCES) and len(seen) == 8
    for inst in LC.SM_INSTANCES[:3] + LC.SM_INSTANCES[6:7]:
        cs = [c for c in cases if c.fwd == inst]
        assert {c.V for c in cs} == set(LC.SM_V), inst
        assert {(c.cs - c.C, c.off) for c in cs} == {(0, 0), (3, 0), (0, 1)}, inst
        assert any(c.noclass and c.V >= 255 for c in cs) and any(c.logits == 'spread' and c.V > 1 for c in cs), inst
    assert {c.C for c in cases} == set(LC.SM_C)
    for c in cases:
        d = LC.sm_draw(c)
        lab = d['labels'].long()
        if c.V >= 255:
            assert set(range(c.C)) <= set(lab.flatten().tolist()), c.id                  # every class
        if c.noclass:
            assert (lab == -1).any() and (lab == c.C).any(), c.id
        if c.logits == 'spread' and c.V > 16:
            x = d['x']
            spread = x.max(2).values - x.min(2).values
            assert int((spread == 200).sum()) >= 3 and int((spread == 160).sum()) >= 3, c.id
            rows = torch.nonzero(spread >= 160)
            at_min = [bool(x[b, v, lab[b, v]] == x[b, v].min()) for b, v in rows.tolist() if 0 <= lab[b, v] < c.C]
            assert any(at_min) and not all(at_min), c.id          # the label's class at the bottom of a row: -log(p) underflows in fp32


def test_softmax_instance_boundaries_and_refusals():
    ops = _ops()
    got = [ops.softmax_dice_ce_kernel_name(Cn, False) for Cn in range(2, 65)]
    want = ['softmax_loss_fwd_kernel<4>'] * 3 + ['softmax_loss_fwd_kernel<8>'] * 4 + ['softmax_loss_fwd_kernel<16>'] * 8 + \
           ['softmax_loss_fwd_wide_kernel'] * 48
    assert got == want
    assert [ops.softmax_dice_ce_kernel_name(Cn, True) for Cn in range(2, 65)] == [w.replace('fwd', 'bwd') for w in want]
    from multitalent_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    for Cn in (1, 0, 65, -3):
        assert lib.mt_softmax_dice_ce_kernel_name(Cn, 0, buf, 128) == -1 and lib.mt_softmax_dice_ce_kernel_name(Cn, 1, buf, 128) == -1
    assert b'2 <= C <= 64' in lib.mt_last_error()
    assert lib.mt_softmax_dice_ce_kernel_name(4, 0, None, 0) == -1


# ---- MultiTalent: names, rule, census, geometry ----------------------------------------------------------------------------------
HAND = {   # a hand-written handful: id -> (forward, backward, bodies, voxels per block forward, blocks forward)
    'c47-v1200-dense-few-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'SSS', 1200, 1),
    'c47-v1201-dense-few-scaled': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_flat_kernel', 'SSS', 1200, 2),
    'c47-v2420-off1-high-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_flat_kernel', 'SSF', 1200, 3),
    'c47-v2416-strided-n23_24-scaled': ('mt_loss_fwd_kernel', 'mt_loss_bwd_kernel', '---', 1024, 3),
    'c47-v2406-dcs-none_all-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_kernel', 'FF', 1200, 3),
    'c47-v2420-dense-n23_24-randn': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'SFF', 1200, 3),
    'c1-v4096-dense-few-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_flat_kernel', 'SFS', 4096, 1),
    'c64-v964-dense-all64-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'FS', 960, 2),
    'c63-v964-dense-all64-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'FS', 960, 2),
    'c16-v3844-dense-all64-planted': ('mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'SS', 3840, 2),
}


def test_multitalent_cases_are_the_kernels_they_claim():
    ops = _ops()
    cases = LC.mt_cases()
    assert len({c.id for c in cases}) == len(cases)
    byid = {c.id: c for c in cases}
    seen = set()
    for c in cases:
        la, da = _addr(c.off), _addr(c.off)
        f = ops.multitalent_loss_fwd_kernel_name(c.cs, c.V, c.C)
        b = ops.multitalent_loss_bwd_kernel_name(la, c.cs, da, c.dcs, c.V, c.C)
        assert f == LC.mt_fwd_rule(c.cs, c.V, c.C) and f[0] == c.fwd, (c.id, f)
        assert b == LC.mt_bwd_rule(la, c.cs, da, c.dcs, c.V, c.C) and b[0] == c.bwd, (c.id, b)
        assert len(c.bodies) == len(c.masks)
        for m, body in zip(c.masks, c.bodies):                      # the per-sample rule of mt_loss_fwd_sparse_kernel, restated
            n = sum((m >> ch) & 1 for ch in range(c.C))
            assert body == ('-' if c.fwd == 'mt_loss_fwd_kernel' else 'S' if 1 <= n <= 23 else 'F'), c.id
        seen |= {c.fwd, c.bwd}
    assert seen == MT_NAMES
    for cid, (fwd, bwd, bodies, vpb, nblk) in HAND.items():
        c = byid[cid]
        assert (c.fwd, c.bwd, c.bodies) == (fwd, bwd, bodies), cid
        assert ops.multitalent_loss_fwd_kernel_name(c.cs, c.V, c.C) == (fwd, vpb, nblk), cid


def test_multitalent_census_lists_five_kernels_and_the_alignment_clause():
    """every (C, cs, alignment, V * C mod 4): the names, and where each backward is taken"""
    ops = _ops()
    names = set()
    for Cn in range(1, 65):
        for cs in (Cn, Cn + 3):
            for la in (LC.FAKE_BASE, LC.FAKE_BASE + 4, LC.FAKE_BASE + 8):
                for da in (LC.FAKE_BASE, LC.FAKE_BASE + 4):
                    for V in (8, 9, 10, 11):
                        f = ops.multitalent_loss_fwd_kernel_name(cs, V, Cn)
                        b = ops.multitalent_loss_bwd_kernel_name(la, cs, da, cs, V, Cn)
                        assert f == LC.mt_fwd_rule(cs, V, Cn) and b == LC.mt_bwd_rule(la, cs, da, cs, V, Cn)
                        wide = cs == Cn and Cn >= 2 and (V * Cn) % 4 == 0 and la % 16 == 0 and da % 16 == 0
                        assert (b[0] == 'mt_loss_bwd_wide_kernel') == wide
                        assert (b[0] == 'mt_loss_bwd_kernel') == (cs != Cn) == (f[0] == 'mt_loss_fwd_kernel')
                        names |= {f[0], b[0]}
        vpb = ops.multitalent_loss_fwd_kernel_name(Cn, 1, Cn)[1]
        nsub = 256 // Cn
        assert vpb == min(240 * nsub, 4096) and vpb % 4 == 0         # the launcher's (vpb * C) & 3 clause never holds
    assert names == MT_NAMES
    assert ops.multitalent_loss_bwd_kernel_name(LC.FAKE_BASE, 47, LC.FAKE_BASE, 50, 8, 47)[0] == 'mt_loss_bwd_kernel'       # dcs != C alone
    from multitalent_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    base = C.c_void_p(LC.FAKE_BASE)
    for cs, V, Cn in ((47, 0, 47), (65, 8, 65), (0, 8, 0)):
        assert lib.mt_multitalent_loss_fwd_kernel_name(cs, V, Cn, buf, 128, None, None) == -1
        assert lib.mt_multitalent_loss_bwd_kernel_name(base, cs, base, cs, V, Cn, buf, 128, None, None) == -1
    assert lib.mt_multitalent_loss_bwd_kernel_name(None, 47, base, 47, 8, 47, buf, 128, None, None) == -1
    assert lib.mt_multitalent_loss_bwd_kernel_name(base, 47, None, 47, 8, 47, buf, 128, None, None) == -1
    assert lib.mt_multitalent_loss_fwd_kernel_name(47, 8, 47, None, 0, None, None) == -1
    assert lib.mt_multitalent_loss_fwd_kernel_name(47, 8, 47, buf, 128, None, None) == 0 and buf.value == b'mt_loss_fwd_sparse_kernel'


def test_multitalent_table_has_every_axis():
    ops = _ops()
    cases = LC.mt_cases()
    assert {c.C for c in cases} == {1, 2, 3, 5, 15, 16, 47, 63, 64}
    assert [LC.lf_nsub(Cn) for Cn in LC.MT_C] == [256, 128, 85, 51, 17, 16, 5, 4, 4]
    assert [LC.lf_vpb(Cn) for Cn in LC.MT_C] == [4096, 4096, 4096, 4096, 4080, 3840, 1200, 960, 960]
    for Cn in LC.MT_C:
        cs = [c for c in cases if c.C == Cn]
        nsub, vpb = LC.lf_nsub(Cn), ops.multitalent_loss_fwd_kernel_name(Cn, 1, Cn)[1]
        vs = {c.V for c in cs if c.cs == Cn}
        want = {1, vpb - 1, vpb, vpb + 1} | ({nsub - 1} if nsub > 1 else set())
        assert want <= {c.V for c in cs}, (Cn, want - vs)
        tails = {(c.V - 2 * vpb) % (4 * nsub) for c in cs if 2 * vpb < c.V < 3 * vpb}
        assert {1 % (4 * nsub), nsub % (4 * nsub), nsub + 1, 3 * nsub + 1} <= tails, (Cn, tails)     # the four-way unroll's tail
        for c in cs:                                                 # the partial last block a case claims
            name, v, nblk = ops.multitalent_loss_fwd_kernel_name(c.cs, c.V, c.C)
            assert nblk == -(-c.V // v) and (nblk - 1) * v < c.V <= nblk * v
        assert any(c.V > 2 * vpb and c.V % vpb for c in cs if c.cs == Cn) and any(c.V > 1024 and c.V % 1024 for c in cs if c.cs != Cn)
        assert {(c.cs - Cn, c.dcs - Cn, c.off) for c in cs} == {(0, 0, 0), (0, 0, 1), (3, 3, 0), (0, 3, 0)}
        dense = [c for c in cs if (c.cs, c.dcs, c.off) == (Cn, Cn, 0)]
        assert any((c.V * Cn) % 4 == 0 for c in dense)
        if Cn % 4:
            assert any((c.V * Cn) % 4 for c in dense) and any(c.bwd == 'mt_loss_bwd_flat_kernel' for c in dense)
        if Cn >= 2:                                                  # the flat backward through the alignment clause alone
            assert any(c.off == 1 and c.cs == c.dcs == Cn and (c.V * Cn) % 4 == 0 and c.bwd == 'mt_loss_bwd_flat_kernel' for c in cs)
            assert any(c.bwd == 'mt_loss_bwd_wide_kernel' for c in cs)
        assert any(c.V < nsub for c in cs) or nsub <= 5
        # the last voxel of the last block in every slot of the four-way unroll: flat forward body, flat backward
        assert {LC.mt_last_slot(c, nsub) for c in cs if 'F' in c.bodies} == {0, 1, 2, 3}, Cn
        assert {LC.mt_last_slot(c, nsub) for c in cs if c.bwd == 'mt_loss_bwd_flat_kernel'} == {0, 1, 2, 3}, Cn
        assert {c.logits for c in cs} == set(LC.MT_LOGITS) and {c.maskname for c in cs} == set(LC.MT_MASKS)
        counts = {LC.popcount(m & LC.mask_of(Cn)) for c in cs for m in c.masks}
        assert {0, 1, Cn} <= counts and (Cn < 3 or {2, 3} <= counts)
        if Cn >= 24:
            assert any({23, 24} <= {LC.popcount(m) for m in c.masks} and 'S' in c.bodies and 'F' in c.bodies for c in cs)
        if Cn < 64:
            assert any(m >> Cn for c in cs for m in c.masks)           # bits at or above C
    sparse = {LC.mt_last_slot(c, 256 // LC.popcount(m & LC.mask_of(c.C))) for c in cases for m, body in zip(c.masks, c.bodies) if body == 'S'}
    assert sparse == {0, 1, 2, 3}
    assert any(c.C == 64 and any(m >> 63 for m in c.masks) for c in cases)
    assert any(c.C == 63 and (1 << 64) - 1 in c.masks for c in cases)
    lut = LC.mt_lut(47)
    assert any(w & 1 and w >> 63 for w in lut) and any(not w & 1 and not w >> 63 for w in lut)
    c = [c for c in cases if c.V >= 70 and c.logits == 'planted'][0]
    d = LC.mt_draw(c)
    labs = set(d['labels'].flatten().tolist())
    assert {-1.0, 0.0, 63.0, 64.0, 200.0, -300.0} <= labs and set(float(v) for v in range(64)) <= labs
    x = d['x']
    for val in (30.0, 88.0, 95.0, 104.0):
        assert (x == val).any() and (x == -val).any()
    z = x[x == 0]
    assert z.numel() and torch.signbit(z).any() and not torch.signbit(z).all()            # +0.0 and -0.0
    sc = LC.mt_draw([c for c in cases if c.logits == 'scaled' and c.C == 47 and c.V >= 70][0])['x']
    row = sc[sc.abs().amax(2) == 104.0][0]                          # a planted row, scaled by channel: +-104 (c + 1) / C
    assert abs(float(row[46])) == 104.0 and abs(abs(float(row[0])) - 104.0 / 47) < 1e-5 and abs(abs(float(row[22])) - 104.0 * 23 / 47) < 1e-4
    assert float(x.abs().max()) == 104.0 and float(sc.abs().max()) == 104.0
    assert len(cases) <= 200


# ---- hard statistics -------------------------------------------------------------------------------------------------------------
def test_hard_stats_construction_leaves_out_no_voxel():
    cases = LC.hs_cases()
    assert len(cases) == 30 and {(c.C, c.cs - c.C, c.V) for c in cases} == {(a, b, v) for a in (1, 47, 64) for b in (0, 3) for v in LC.HS_V}
    assert {c.maskname for c in cases} == set(LC.MT_MASKS) and any(0 in c.masks for c in cases)
    for c in cases:
        d = LC.hs_draw(c)
        x = d['x']
        assert LC.hs_left_out(x) == 0, c.id                        # the cap is 0 voxels left out
        assert c.V == 1 or float(x[x != 0].abs().min()) >= np.float32(LC.HS_EPS)
        z = x[x == 0]
        assert z.numel() > 0
        if c.C > 1 and c.V > 1:
            assert torch.signbit(z).any() and not torch.signbit(z).all()
        ref = LC.hs_reference(x, d['labels'], d['masks'], d['lut'])
        assert ref.dtype == np.int64 and ref.shape == (len(c.masks), c.C, 3)
        # the same counts from the soft reference's targets, one sample and channel at a time
        y = LC.mt_targets(d['labels'], d['lut']).bool()
        for b, m in enumerate(c.masks):
            for ch in (0, c.C // 2, c.C - 1):
                p = x[b, :, ch] > 0
                want = [int((p & y[b, :, ch]).sum()), int((p & ~y[b, :, ch]).sum()), int((~p & y[b, :, ch]).sum())] if (m >> ch) & 1 else [0, 0, 0]
                assert ref[b, ch].tolist() == want, (c.id, b, ch)
    # fp32 sigmoid at the edge of the construction decides as x > 0 does, and 0 is not predicted
    e = np.float32(LC.HS_EPS)
    ex = np.exp(-e, dtype=np.float32)
    assert np.float32(1) / (np.float32(1) + ex) > np.float32(0.5) + np.float32(1e-4) and ex / (np.float32(1) + ex) < np.float32(0.5) - np.float32(1e-4)
    assert not (np.float32(1) / (np.float32(1) + np.float32(1)) > np.float32(0.5))


# ---- combination -----------------------------------------------------------------------------------------------------------------
def test_combine_reference_is_the_oracle_loss():
    """MultiTalent: statistics of the float64 reference through cb_reference == oracle.reference_ops.multitalent_loss; batch Dice:
    cb_reference over the batch == oracle.reference_ops.soft_dice_loss(batch_dice=True)"""
    from oracle import reference_ops as R
    g = LC.gen('oracle')
    B, Cn, shapes, w = 3, 5, [(4, 6, 5), (2, 3, 5)], [0.6, 0.4]
    regions = {'a': (1,), 'b': (2, 3), 'c': (1, 2, 3, 7), 'd': (63,), 'e': (0, 5)}
    idx = {'a': 0, 'b': 1, 'c': 2, 'd': 3, 'e': 4}
    valid = [['a', 'c'], ['b'], ['a', 'b', 'd', 'e']]
    lut = [sum(1 << l for l in regions[n]) for n in 'abcde']
    masks = [sum(1 << idx[r] for r in v) for v in valid]
    outs = [torch.randn((B, Cn) + s, generator=g).double() * 2 for s in shapes]
    tgs = [torch.randint(0, 8, (B, 1) + s, generator=g).float() for s in shapes]
    want = R.multitalent_loss(outs, tgs, valid, regions, idx, w, batch_dice=True)
    stats = torch.stack([LC.mt_reference(o.reshape(B, Cn, -1).permute(0, 2, 1), t.reshape(B, -1), masks, lut)[0] for o, t in zip(outs, tgs)])
    ce_coef = torch.tensor([wi / float(np.prod(s)) for wi, s in zip(w, shapes)], dtype=torch.float64)
    got, grad = LC.cb_reference(stats, 1.0, ce_coef, torch.tensor(w, dtype=torch.float64), LC.CE_ALL, 0, (0.0, 0.0, 0.0, 1e-7))
    assert np.allclose(got, [float(v) for v in want], rtol=1e-9, atol=1e-12), (got, want)
    # regions a sample does not carry: ratio 0 / clamp, gradient -k * 2 / clamp_min on tp and 0 on fp, fn
    l, b, ch = 1, 1, 0
    assert float(stats[l, b, ch].abs().max()) == 0.0
    assert abs(float(grad[l, b, ch, 1]) + 0.4 * 2 / LC.f32(1e-7)) < 1e-3 and grad[l, b, ch, 2:].abs().max() == 0
    # nnU-Net's batch Dice without background
    x = torch.randn((B, Cn, 4, 6, 5), generator=g).double()
    t = torch.randint(0, Cn, (B, 1, 4, 6, 5), generator=g).float()
    st = LC.sm_reference(x.reshape(B, Cn, -1).permute(0, 2, 1), t.reshape(B, -1))[0][None]
    got, _ = LC.cb_reference(st, 1.0, torch.zeros(1, dtype=torch.float64), torch.full((1,), 1.0 / (Cn - 1), dtype=torch.float64), LC.OVER_B, 1,
                             (1e-5, 1e-5, 1e-8, -3e38))
    want = float(R.soft_dice_loss(x, t, batch_dice=True, do_bg=False, smooth=LC.f32(1e-5)))
    assert abs(got[0] - want) < 1e-9 and got[1] == 0.0


def test_combine_table():
    cases = LC.cb_cases()
    assert len({c.id for c in cases}) == len(cases) == 40
    assert sorted({c.L * c.B * c.C for c in cases}) == [2, 141, 252, 258, 940]
    assert {(c.flags, c.c0) for c in cases} == {(f, z) for f in range(4) for z in (0, 1)}
    assert {(c.stride, c.consts) for c in cases} == {(s, n) for s in (3, 4) for n in LC.CB_CONSTS}
    n_over = {c.L * (1 if c.flags & 2 else c.B) * (c.C - c.c0) for c in cases}
    assert min(n_over) < 256 < max(n_over) and any(c.flags & 2 and c.L * (c.C - c.c0) < 256 < c.L * c.B * (c.C - c.c0) for c in cases)
    for c in cases[::7]:
        d = LC.cb_draw(c)
        st = d['stats']
        nz = st[st != 0]
        assert st.dtype == torch.float32 and float(nz.max()) <= 1.8e6 * 1.001 and (d['rows']['zero'] or c.L * c.B * c.C < 8)
        assert all(float(st.view(-1, 4)[i].abs().max()) == 0.0 for i in d['rows']['zero'])
        k = d['k']
        assert k == (1.0 if c.stride == 4 else 2.0)
        if d['rows']['below'] is not None:
            raw = [k * float(2 * st.view(-1, 4)[i, 1].double() + st.view(-1, 4)[i, 2].double() + st.view(-1, 4)[i, 3].double()) for i in (1, 2)]
            assert 0.4e-7 < raw[1] < 0.6e-7 < LC.f32(1e-7) < 1.4e-7 < raw[0] < 1.6e-7 and float(st.view(-1, 4)[2, 1]) > 0


# ---- optimizer -------------------------------------------------------------------------------------------------------------------
def test_sgd_reference_is_torch_sgd_with_clip_grad_norm():
    lr, wd, mom, mx = LC.SG_HP
    g = LC.gen('torch-sgd')
    n = 1000
    for scale in (0.01, 0.5, 40.0):                                  # norms below and above max_norm
        p0 = torch.randn(n, generator=g).double()
        pr = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([pr], LC.f32(lr), weight_decay=LC.f32(wd), momentum=LC.f32(mom), nesterov=True)
        p, buf = p0.clone(), torch.randn(n, generator=g).double()
        for step in range(3):
            gr = torch.randn(n, generator=g).double() * scale
            pr.grad = gr.clone()
            torch.nn.utils.clip_grad_norm_([pr], LC.f32(mx))
            opt.step()
            p, buf = LC.sg_reference(p, buf, gr, step == 0, float((gr ** 2).sum()))
            assert torch.allclose(p, pr.detach(), rtol=1e-12, atol=1e-13), (scale, step)
    # without a norm: plain SGD; an infinite norm: a pure weight-decay step
    p1, b1 = LC.sg_reference(p0, buf, gr, True, None)
    assert torch.allclose(b1, gr + LC.f32(wd) * p0)
    p2, b2 = LC.sg_reference(p0, buf, gr, True, float('inf'))
    assert torch.allclose(b2, LC.f32(wd) * p0) and torch.allclose(p2, p0 - LC.f32(lr) * (1 + LC.f32(mom)) * LC.f32(wd) * p0)


def test_optimizer_tables_and_refusals():
    assert [c.n for c in LC.ss_cases()][:11] == [1, 2, 3, 4, 5, 7, 4095, 4096, 4097, 100003, 4194304 + 4099]
    assert {c.n & 3 for c in LC.ss_cases()} == {0, 1, 2, 3}
    assert (4194304 + 4099) // 4 > 1024 * 256 * 4 and 2097152 + 1027 > 2048 * 256 * 4             # past the block caps: one more trip
    x = LC.ss_draw([c for c in LC.ss_cases() if c.big == 1e18][0])
    assert np.isfinite(np.float32(LC.ss_reference(x))) and LC.ss_reference(x) > 0.999e36
    x = LC.ss_draw([c for c in LC.ss_cases() if c.big == 1e20][0])
    assert LC.ss_reference(x) > 3.5e38                           # beyond fp32
    sg = LC.sg_cases()
    assert [c.n for c in sg] == [1, 255, 1025, 100003, 2097152 + 1027]
    for pos in range(3):
        assert {c.steps[pos] for c in sg} == {None, 'below', 'above', 'far', 'inf'}
    mx = LC.SG_HP[3]
    assert np.sqrt(LC.sg_sumsq('below')) < mx < np.sqrt(LC.sg_sumsq('above')) < 1.01 * mx and np.sqrt(LC.sg_sumsq('far')) > 1e3 * mx
    # the refusals are host decisions: no device is touched before them
    from multitalent_amd import _lib
    lib = _lib.load()
    base, out, ws = C.c_void_p(LC.FAKE_BASE), C.c_void_p(LC.FAKE_BASE + 4096), C.c_void_p(LC.FAKE_BASE + 8192)
    need = lib.mt_sumsq_workspace(100)
    assert need == 4096
    assert lib.mt_sumsq(C.c_void_p(LC.FAKE_BASE + 4), 100, out, ws, need, None) == -1 and b'16-byte' in lib.mt_last_error()
    assert lib.mt_sumsq(base, 100, out, ws, need - 4, None) == -2 and b'workspace' in lib.mt_last_error()
    assert lib.mt_sumsq(base, 100, out, None, need, None) == -2
    assert lib.mt_sumsq(base, 0, out, ws, need, None) == -1


def test_bounds_are_never_looser_than_the_projects():
    print(LC.bounds_text())
    assert (LC.MT_STATS_RTOL, LC.MT_STATS_ATOL, LC.MT_GRAD_RTOL, LC.MT_GRAD_ATOL) == (2e-5, 1e-3, 1e-4, 1e-5)
    assert (LC.SM_STATS_REL, LC.SM_STATS_ABS, LC.SM_GRAD, LC.SGD_RELERR) == (1e-4, 1e-4, 1e-5, 1e-6)
    assert LC.SUMSQ_MULT * LC.U < 1e-4 and max(LC.COMBINE_VALUE_MULT, LC.COMBINE_GRAD_MULT) * LC.U <= 2e-6
    assert max(LC.mt_chain(c) for c in LC.mt_cases()) <= 16 + 256 and min(LC.mt_chain(c) for c in LC.mt_cases()) >= 64
