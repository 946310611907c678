"""State of multitalent_amd/engine.py that outlives a call: the call sequences of tests/engine_cases.SEQUENCES on ONE
engine, each held to a FRESH engine — the same network built again from the same seed and taken to the same final state directly.
Every reduction of the engine has a fixed order (test_training_step_is_bit_reproducible_at_full_size), so the yardstick is torch.equal
on the logits and on every gradient; where two settings legitimately reorder sums (fuse_norm_bwd on against off) it is the 2e-5 of
the tensor's largest entry of test_fused_norm_backward_statistics_through_the_engine; where the sequence changes the weights the
second yardstick is the fp64 oracle taken through the same steps (compare())."""
import copy

import numpy as np
import pytest
import torch

import engine_cases as EC
from test_engine_paths_gpu import Recorder, fresh_net, hip_loss, hip_step, set_ds

pytestmark = pytest.mark.gpu

SEQ = {s['name']: s for s in EC.SEQUENCES}
SHAPES = [(2, (8, 16, 16)), (1, (8, 32, 16)), (3, (16, 16, 16))]


def items(name):
    s = SEQ[name]
    out = [(c, 'fp32') for c in s['on']]
    if s['mixed']:
        out += [(c, 'bf16') for c in s['on']]
    return pytest.mark.parametrize('base,precision', out, ids=['%s-%s' % i for i in out])


def config(base, precision='fp32', **kw):
    return dict(EC.CONFIG[base], precision=precision, **kw)


def same(a, b, what):
    (la, lossa, ga), (lb, lossb, gb) = a, b
    assert len(la) == len(lb)
    for i, (u, v) in enumerate(zip(la, lb)):
        assert torch.equal(u, v), "%s: logits of level %d differ by %.3e" % (what, i, float((u - v).abs().max()))
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None), (what, n)
        if ga[n] is not None:
            assert torch.equal(ga[n], gb[n]), "%s: gradient of %s differs by %.3e" % (what, n, float((ga[n] - gb[n]).abs().max()))


@pytest.fixture
def sixteen_bit_kernels_here():
    """the 16-bit kernels also on these small grids (as tests/test_mixed_precision_gpu.py), restored for the autouse check"""
    from multitalent_amd import ops
    ops.set_option('conv_bf16', 2)
    yield
    ops.set_option('conv_bf16', 1)
    ops.set_option('conv_wino', 1)
    ops.set_mma(0)


def case_at(cfg, i):
    B, shape = SHAPES[i]
    return EC.make_case(cfg, shape, B, seed=20 + i)


def perturbed_state(cfg):
    """`other`: the state of the same architecture with every parameter moved"""
    net, _ = EC.build_net(cfg)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


# ---- 1
@items('stock-optimizer')
def test_stock_optimizer(dev, base, precision):
    """a stock torch optimizer and NO mark_params_dirty(): the second iteration must run on the stepped weights"""
    cfg = config(base)
    cases = [case_at(cfg, 0), EC.make_case(cfg, SHAPES[0][1], SHAPES[0][0], seed=31)]
    sd0 = {k: v.detach().clone() for k, v in EC.build_net(cfg)[0].state_dict().items()}
    for kind, make_opt in (('SGD', lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.99, nesterov=True)),
                           ('AdamW', lambda ps: torch.optim.AdamW(ps, lr=1e-3))):
        def loop(mark):
            net = fresh_net(cfg, dev)
            opt = make_opt(list(net.parameters()))          # created BEFORE the parameters are re-homed into the flat buffer
            for i, case in enumerate(cases):
                res = hip_step(cfg, net, case, dev)
                if i + 1 < len(cases):
                    opt.step()
                    if mark:
                        net.engine().mark_params_dirty()
            return res
        plain, marked = loop(False), loop(True)
        o32 = EC.oracle_train(cfg, torch.float32, sd0, cases, make_opt)
        o64 = EC.oracle_train(cfg, torch.float64, sd0, cases, make_opt)
        print("ENGINE-FIG stock-optimizer %s %s: HIP rel. L2 %.2e, fp32 oracle %.2e, cos %.8f, worst %.3f (%s)"
              % ((base, kind) + EC.figures(plain[2], o32, o64)))
        same(plain, marked, '%s without mark_params_dirty() against with' % kind)
        EC.compare('%s %s iteration 2' % (base, kind), plain[0], plain[1], plain[2], o32, o64)


# ---- 2
@items('load-state-dict')
def test_load_state_dict(dev, base, precision):
    cfg = config(base)
    case, other = case_at(cfg, 0), perturbed_state(cfg)
    net = fresh_net(cfg, dev)
    first = hip_step(cfg, net, case, dev)
    net.load_state_dict(other)                               # and nothing else
    second = hip_step(cfg, net, case, dev)
    ref = fresh_net(cfg, dev)
    ref.load_state_dict(other)
    want = hip_step(cfg, ref, case, dev)
    assert not torch.equal(first[0][0], want[0][0])           # (the two states do differ)
    same(second, want, 'after load_state_dict against a fresh network loaded with the same state')
    # a write no version counter sees (through p.data), announced with mark_params_dirty() as INTEGRATION.md §2 asks
    for p in net.parameters():
        p.data.mul_(0.5)
    net.engine().mark_params_dirty()
    third = hip_step(cfg, net, case, dev)
    ref = fresh_net(cfg, dev)
    ref.load_state_dict({k: 0.5 * v for k, v in other.items()})
    assert not torch.equal(third[0][0], second[0][0])
    same(third, hip_step(cfg, ref, case, dev), 'after p.data.mul_() + mark_params_dirty() against a fresh network with those weights')


# ---- 3
@items('shape-roundtrip')
def test_shape_roundtrip(dev, base, precision, sixteen_bit_kernels_here):
    cfg = config(base, precision)
    net = fresh_net(cfg, dev)
    got = []
    for i in (0, 1, 2, 0):
        got.append(hip_step(cfg, net, case_at(cfg, i), dev))
        same(got[-1], hip_step(cfg, fresh_net(cfg, dev), case_at(cfg, i), dev), 'step %d at %s against a fresh engine' % (len(got), SHAPES[i]))
    same(got[3], got[0], 'the first shape again')


# ---- 4
@items('train-validate-train')
def test_train_validate_train(dev, base, precision, monkeypatch, sixteen_bit_kernels_here):
    from multitalent_amd.inference.sliding_window import predict_3D
    cfg = config(base, precision)
    case = case_at(cfg, 0)
    g = torch.Generator().manual_seed(41)
    xv = torch.randn((1, cfg['in_ch'], 8, 32, 16), generator=g).to(dev)
    vol = torch.randn((cfg['in_ch'], 12, 40, 24), generator=g).numpy()

    def validate(net):
        net.eval()
        set_ds(net, False)
        with torch.no_grad():
            whole = net(xv).detach().float().cpu().clone()
        seg, probs = predict_3D(net, vol, True, (0, 1, 2), True, 0.5, (8, 16, 16), use_gaussian=True, verbose=False,
                                mixed_precision=precision == 'bf16')
        net.train()
        set_ds(net, True)
        return whole, seg.copy(), probs.copy()

    net = fresh_net(cfg, dev)
    first = hip_step(cfg, net, case, dev)
    rec = Recorder(monkeypatch)
    got = validate(net)
    monkeypatch.undo()
    assert 'heads:skip-final' in rec.tags, sorted(rec.tags)           # the tiled prediction went through forward_to_final_head
    again = hip_step(cfg, net, case, dev)
    same(again, first, 'the train step after validation against the one before')
    want = validate(fresh_net(cfg, dev))
    assert torch.equal(got[0], want[0]), float((got[0] - want[0]).abs().max())
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- 5
@items('nograd-in-train-mode')
def test_nograd_in_train_mode(dev, base, precision):
    cfg = config(base)
    net = fresh_net(cfg, dev)
    with torch.no_grad():
        assert net.training
        out = net(case_at(cfg, 1)['x'].to(dev))
        assert not out[0].requires_grad
    same(hip_step(cfg, net, case_at(cfg, 0), dev), hip_step(cfg, fresh_net(cfg, dev), case_at(cfg, 0), dev),
         'a step after a no_grad forward in train mode against a fresh engine')


# ---- 6
@items('precision-roundtrip')
def test_precision_roundtrip(dev, base, precision, sixteen_bit_kernels_here):
    cfg = config(base)
    case = case_at(cfg, 0)
    net = fresh_net(cfg, dev)
    got = []
    for mode in ('fp32', 'bf16', 'fp32'):
        net.engine().set_precision(mode)
        got.append(hip_step(cfg, net, case, dev))
    same(got[2], got[0], 'fp32 after bf16 against fp32 before')
    same(got[1], hip_step(cfg, fresh_net(config(base, 'bf16'), dev), case, dev), 'bf16 on a used engine against a fresh bf16 engine')
    assert not torch.equal(got[1][0][0], got[0][0][0])


# ---- 7
@items('stream-and-fuse-switch')
def test_stream_and_fuse_switch(dev, base, precision, monkeypatch):
    from multitalent_amd import ops
    cfg = config(base)
    case = case_at(cfg, 0)
    ops.set_option('conv_wino', 2)                  # the Winograd forms, the ones that fuse, also at this size
    try:
        net = fresh_net(cfg, dev)
        eng = net.engine()
        first = None
        for streams in (1, 0, 0, 2, 1):
            eng.bwdw_streams = streams
            with torch.no_grad():                   # new weights: the packing programs run again under every setting (twice under 0)
                for p in net.parameters():
                    p.mul_(1.0)
            rec = Recorder(monkeypatch)
            res = hip_step(cfg, net, case, dev)
            monkeypatch.undo()
            assert 'streams:%d' % streams in rec.tags, (streams, sorted(rec.tags))
            assert ('pack:main-only' in rec.tags) == (streams == 0), (streams, sorted(rec.tags))
            first = first or res
            same(res, first, 'bwdw_streams = %d against 1' % streams)
        for fuse in (None, 1, 0, 3):
            eng.fuse_norm_bwd = fuse
            rec = Recorder(monkeypatch)
            res = hip_step(cfg, net, case, dev)
            monkeypatch.undo()
            assert ('norm-bwd:part' in rec.tags) == (fuse == 1 or (fuse == 3 and cfg['arch'] == 'resenc')), (fuse, sorted(rec.tags))
            assert ('bwdd:stride1:stats' in rec.tags) == (fuse == 1), (fuse, sorted(rec.tags))
            assert ('resadd:stats' in rec.tags) == (fuse in (1, 3) and cfg['arch'] == 'resenc'), (fuse, sorted(rec.tags))
            for u, v in zip(res[0], first[0]):
                assert torch.equal(u, v)
            for n, b in first[2].items():
                assert float((res[2][n] - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-3), (fuse, n)
    finally:
        ops.set_option('conv_wino', 1)


# ---- 8
@items('accumulate-grads')
def test_accumulate_grads(dev, base, precision):
    cfg = config(base)
    c1, c2 = case_at(cfg, 0), EC.make_case(cfg, SHAPES[0][1], SHAPES[0][0], seed=32)
    ref = fresh_net(cfg, dev)
    g1, g2 = hip_step(cfg, ref, c1, dev)[2], hip_step(cfg, ref, c2, dev)[2]
    net = fresh_net(cfg, dev)
    hip_step(cfg, net, c1, dev)
    got = hip_step(cfg, net, c2, dev, zero_grad=False)[2]
    fg = net.engine().flat_grad
    lo, hi = fg.data_ptr(), fg.data_ptr() + 4 * fg.numel()
    for n, p in net.named_parameters():
        assert torch.equal(got[n], g1[n] + g2[n]), n
        assert not (lo <= p.grad.data_ptr() < hi), "%s.grad aliases the flat gradient buffer, which the next backward zeroes" % n


# ---- 9
@items('stale-backward')
def test_stale_backward(dev, base, precision):
    """returned logits alias engine buffers that the next forward overwrites — so a backward through the earlier
    forward would silently be the later one's; engine._UNetFunction refuses it"""
    cfg = config(base)
    c1, c2 = case_at(cfg, 0), EC.make_case(cfg, SHAPES[0][1], SHAPES[0][0], seed=33)
    net = fresh_net(cfg, dev)
    out1 = net(c1['x'].to(dev))
    l1 = hip_loss(cfg, out1, c1, dev)[0]
    out2 = net(c2['x'].to(dev))
    with pytest.raises(RuntimeError, match="a later forward of the same network has overwritten"):
        l1.backward()
    assert all(p.grad is None for p in net.parameters())
    ls = hip_loss(cfg, out2, c2, dev)
    ls[0].backward()
    torch.cuda.synchronize()
    want = hip_step(cfg, fresh_net(cfg, dev), c2, dev)
    got = ([o.detach().float().cpu() for o in out2], [float(l.detach()) for l in ls],
           {n: p.grad.detach().cpu() for n, p in net.named_parameters()})
    same(got, want, 'backward of the latest forward against a fresh engine')


# ---- 10
@items('frozen-body')
def test_frozen_body(dev, base, precision):
    cfg = config(base)
    case = case_at(cfg, 0)
    want = hip_step(cfg, fresh_net(cfg, dev), case, dev)
    net = fresh_net(cfg, dev)
    heads = [n for n, _ in net.named_parameters() if n.startswith(('seg_outputs.', 'decoder.deep_supervision_outputs.'))]
    assert heads
    for n, p in net.named_parameters():
        p.requires_grad_(n in heads)
    got = hip_step(cfg, net, case, dev)
    for n in got[2]:
        if n in heads:
            assert torch.equal(got[2][n], want[2][n]), n
        else:
            assert got[2][n] is None, n
    for u, v in zip(got[0], want[0]):
        assert torch.equal(u, v)


# ---- 11
@items('rehome')
def test_rehome(dev, base, precision):
    cfg = config(base)
    case = case_at(cfg, 0)
    want = hip_step(cfg, fresh_net(cfg, dev), case, dev)
    net = fresh_net(cfg, dev)
    hip_step(cfg, net, case_at(cfg, 1), dev)
    net.cpu()
    assert all(not p.is_cuda for p in net.parameters())
    net.to(dev)
    same(hip_step(cfg, net, case, dev), want, 'after net.cpu(); net.to(dev) against a fresh engine')
    twin = copy.deepcopy(net)
    assert twin.engine() is not net.engine()
    same(hip_step(cfg, twin, case, dev), want, 'copy.deepcopy(net) against a fresh engine')
    for p in twin.parameters():
        assert torch.equal(twin.engine().grad_of(p), p.grad)
    own = {id(p) for p in net.parameters()}
    assert not any(id(p) in own for p in twin.parameters())
    same(hip_step(cfg, net, case, dev), want, 'the original after its copy ran')


# ---- 12
@items('ds-toggle')
def test_ds_toggle(dev, base, precision, monkeypatch):
    cfg, off = config(base), config(base, ds=False)
    case = case_at(cfg, 0)
    net = fresh_net(cfg, dev)
    on1 = hip_step(cfg, net, case, dev)
    set_ds(net, False)
    rec = Recorder(monkeypatch)
    mid = hip_step(off, net, case, dev)
    monkeypatch.undo()
    assert {'heads:final-only-grad', 'head:skipped'} <= rec.tags, sorted(rec.tags)
    set_ds(net, True)
    on2 = hip_step(cfg, net, case, dev)
    same(on2, on1, 'deep supervision on again against the first step')
    same(mid, hip_step(off, fresh_net(off, dev), case, dev), 'deep supervision off on a used engine against a fresh one')
    same(on1, hip_step(cfg, fresh_net(cfg, dev), case, dev), 'the first step against a fresh engine')


def test_every_sequence_has_its_test():
    have = {n[len('test_'):].replace('_', '-') for n in globals() if n.startswith('test_')}
    assert {s['name'] for s in EC.SEQUENCES} <= have
