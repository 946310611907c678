"""multitalent_amd/engine.py, branch by branch: every configuration of tests/engine_cases.py runs forward, loss and
backward through net(x) and loss.backward() — the autograd seam, engine._UNetFunction — under a recorder that observes which entry
points the engine called and with which struct fields, and the result is held to compare() (fp32) or to the bounds of
tests/test_mixed_precision_gpu.py (mixed precision).  The recorded tags must contain the configuration's `expects`: a gradient that
is right although the branch under test never ran proves nothing about that branch."""
import pytest
import torch

import engine_cases as EC

pytestmark = pytest.mark.gpu


class Recorder:
    """Observes the engine's calls (it wraps them with monkeypatch and restores them with it) and maps what it saw to the tags of
    engine_cases.BRANCHES.  It reads struct fields and arguments; it does not restate the engine's conditions."""

    def __init__(self, monkeypatch):
        from multitalent_amd import _lib, engine as G, ops
        self.tags = set()
        self.stack = []                 # (op, 'fwd' | 'bwd'), innermost last (HeadOp.backward may call ConvNormOp.backward)
        self.G, self.ops = G, ops
        mp = monkeypatch
        for cls in (G.ConvNormOp, G.HeadOp, G.TConvOp, G.ResAddOp, G._MaterialiseOp):
            for meth, phase in (('forward', 'fwd'), ('backward', 'bwd')):
                if meth in cls.__dict__:
                    mp.setattr(cls, meth, self._op_method(cls.__dict__[meth], phase))
        for name in ('conv3d_fwd', 'pointwise_fwd', 'conv3d_bwd_data_strided', 'conv3d_bwd_weight', 'head_bwd', 'channel_sum',
                     'inorm_lrelu_bwd', 'ncdhw_to_ndhwc'):
            mp.setattr(ops, name, self._wrap(getattr(ops, name), getattr(self, '_on_' + name)))
        lib = _lib.load()
        for name, tag in (('mt_lrelu_bwd_stats', 'resadd:stats'), ('mt_lrelu_bwd', 'resadd:plain')):
            mp.setattr(lib, name, self._wrap(getattr(lib, name), lambda res, a, kw, tag=tag: self.tags.add(tag)))
        for name in ('zero_', 'add_', 'copy_'):
            mp.setattr(torch.Tensor, name, self._tensor_method(getattr(torch.Tensor, name), name))
        mp.setattr(ops.PackProgram, 'run', self._pack_run(ops.PackProgram.run))
        mp.setattr(G.Engine, '_pack', self._engine_pack(G.Engine._pack))
        mp.setattr(G.Engine, 'forward', self._engine_forward(G.Engine.forward))
        mp.setattr(G.Engine, 'backward', self._engine_backward(G.Engine.backward))
        self.inplace, self.pack_runs, self.side, self.main = [], [], set(), None
        self.ncdhw, self.seen, self.parity, self.heads_run = False, set(), [0, 0], 0

    # ---- wrappers
    @staticmethod
    def _wrap(orig, on):
        def f(*a, **kw):
            res = orig(*a, **kw)
            on(res, a, kw)
            return res
        return f

    def _tensor_method(self, orig, name):
        rec = self

        def f(t, *a, **kw):
            if rec.stack and rec.stack[-1][1] == 'bwd':
                rec.inplace.append((name, t.data_ptr()))
            return orig(t, *a, **kw)
        return f

    def _op_method(self, orig, phase):
        rec = self

        def f(op, eng):
            outer = not rec.stack
            if outer:
                rec.inplace, rec.seen = [], set()
            rec.stack.append((op, phase))
            try:
                return orig(op, eng)
            finally:
                rec.stack.pop()
                if outer:
                    rec._op_done(op, phase)
        return f

    def _op_done(self, op, phase):
        G, kind = self.G, type(op).__name__
        if isinstance(op, G._MaterialiseOp):
            self.seen_mat = getattr(self, 'seen_mat', set()) | {phase}
            if self.seen_mat == {'fwd', 'bwd'}:
                self.tags.add('materialise')
        if phase != 'bwd':
            return
        if isinstance(op, G.ConvNormOp) and not (self.seen & {'bwdd', 'head_bwd'}):
            self.tags.add('bwdd:none')
        if isinstance(op, G.HeadOp):
            self.heads_run += 1
        if 'parity' in self.seen and self.parity[0] < self.parity[1]:
            self.tags.add('bwdd:parity:classes<full')
        if isinstance(op, G.ResAddOp) and op.res.grad is not None:
            ptr = op.res.grad.data_ptr()
            mine = [n for n, q in self.inplace if q == ptr and n in ('add_', 'copy_')]
            if mine:
                self.tags.update('resadd:' + n for n in mine)
            elif ptr == op.out.grad.data_ptr():
                self.tags.add('resadd:shared')

    def _top(self):
        return self.stack[-1] if self.stack else (None, None)

    # ---- entry points
    def _on_conv3d_fwd(self, res, a, kw):
        p, (op, phase), G = a[0], self._top(), self.G
        if phase == 'fwd' and isinstance(op, G.ConvNormOp):
            self.tags.add('fwd:conv')
        elif phase == 'bwd' and isinstance(op, G.TConvOp):
            self.tags.add('tconv:accumulate' if p.accumulate else 'tconv:first-writer')
        elif phase == 'bwd' and isinstance(op, G.ConvNormOp):
            if p.OD:                        # strided placement of the output: one parity class
                if 'parity' not in self.seen:
                    self.parity = [0, p.osD * p.osH * p.osW]
                self.seen |= {'bwdd', 'parity'}
                self.parity[0] += 1
                self.tags.add('bwdd:parity:acc%d' % p.accumulate)
                if any(n == 'zero_' and q == op.srcs[0].grad.data_ptr() for n, q in self.inplace):
                    self.tags.add('bwdd:parity:zero')
            else:
                self.seen.add('bwdd')
                self.tags.add('bwdd:stride1:acc%d' % p.accumulate)
                if p.stats_part:
                    self.tags.add('bwdd:stride1:stats')
                if p.out1:
                    self.tags.add('bwdd:stride1:two-dest')

    def _on_pointwise_fwd(self, res, a, kw):
        p, (op, phase), G = a[0], self._top(), self.G
        if phase == 'fwd' and isinstance(op, G.HeadOp):
            self.tags.add('fwd:head')
        elif phase == 'fwd' and isinstance(op, G.ConvNormOp):
            self.tags.add('fwd:pw_strided')
        elif phase == 'bwd' and isinstance(op, G.ConvNormOp):
            self.seen.add('bwdd')
            if p.scatter:
                zeroed = any(n == 'zero_' and q == op.srcs[0].grad.data_ptr() for n, q in self.inplace)
                self.tags.add('bwdd:pw_strided:zero' if zeroed else 'bwdd:pw_strided:acc')
            else:
                self.tags.add('bwdd:pointwise:acc%d' % p.accumulate)
                if isinstance(op, G.HeadOp):
                    self.tags.add('head:generic')

    def _on_conv3d_bwd_data_strided(self, res, a, kw):
        self.seen.add('bwdd')
        self.tags.add('bwdd:strided:acc%d' % a[0].accumulate)

    def _on_conv3d_bwd_weight(self, res, a, kw):
        s = torch.cuda.current_stream().cuda_stream
        if s != self.main:
            self.side.add(s)

    def _on_head_bwd(self, done, a, kw):
        self.seen.add('head_bwd')
        self.tags.update(('head:fused', 'head:done1' if done else 'head:done0', 'head:accumulate' if a[4] else 'head:first-writer'))

    def _on_channel_sum(self, res, a, kw):
        self.tags.add('head:done0:channel_sum' if 'head_bwd' in self.seen else 'bias:channel_sum')

    def _on_inorm_lrelu_bwd(self, res, a, kw):
        self.tags.add('norm-bwd:part' if kw.get('part') is not None else 'norm-bwd:plain')

    def _on_ncdhw_to_ndhwc(self, res, a, kw):
        self.ncdhw = True

    # ---- engine level
    def _pack_run(self, orig):
        rec = self

        def f(prog):
            rec.pack_runs.append(prog)
            return orig(prog)
        return f

    def _engine_pack(self, orig):
        rec = self

        def f(eng, need_grad):
            rec.pack_runs = []
            orig(eng, need_grad)
            ran = {id(p) for p in rec.pack_runs}
            for main, late, mid, _ in eng._pack_programs.values():
                if not (ran & {id(main), id(late), id(mid)} - {id(None)}):
                    continue
                if late is not None and id(late) in ran:
                    rec.tags.add('pack:late')
                if mid is not None and id(mid) in ran:
                    rec.tags.add('pack:mid')
                if ran == {id(main)}:
                    rec.tags.add('pack:main-only')
        return f

    def _engine_forward(self, orig):
        rec = self

        def f(eng, x, need_grad=True, all_heads=True, _skip_final=False):
            rec.ncdhw = False
            out = orig(eng, x, need_grad=need_grad, all_heads=all_heads, _skip_final=_skip_final)
            rec.tags.add('input:cin>1' if rec.ncdhw else 'input:cin1')
            if _skip_final:
                rec.tags.add('heads:skip-final')
            if need_grad and not all_heads:
                rec.tags.add('heads:final-only-grad')
            return out
        return f

    def _engine_backward(self, orig):
        rec = self

        def f(eng, dlogits):
            from multitalent_amd import _lib
            rec.main, rec.side, rec.heads_run = torch.cuda.current_stream().cuda_stream, set(), 0
            orig(eng, dlogits)
            rec.tags.add('streams:%d' % len(rec.side))
            rec.tags.add('fuse:%d' % eng.fuse_norm_bwd)
            if rec.heads_run < sum(isinstance(o, rec.G.HeadOp) for o in eng.ops):
                rec.tags.add('head:skipped')
            for (key, din, dout), flags in eng._io_cache.items():
                if any(d != _lib.MT_F32 for d in din + dout):
                    rec.tags.add({(False, False): 'io:native', (True, False): 'io:cast-in', (False, True): 'io:cast-out',
                                  (True, True): 'io:cast-both'}[tuple(flags)])
        return f


def hip_loss(cfg, out, case, dev):
    from multitalent_amd.training.loss_functions.fused_losses import DC_and_CE_DS_loss, MultiTalentLoss
    outs = [out] if torch.is_tensor(out) else list(out)
    outs = EC.selected(cfg, outs)
    tg = [t.to(dev) for t in EC.selected(cfg, case['targets'])]
    w = [1.0] if not cfg['ds'] else EC.selected(cfg, case['weights'])
    for o, t in zip(outs, tg):              # (before any loss kernel reads a target through the logits' geometry)
        assert tuple(o.shape[2:]) == tuple(t.shape[2:]) and o.shape[0] == t.shape[0] and o.shape[1] == cfg['nc'], (o.shape, t.shape)
    if cfg['loss'] == 'multitalent':
        return tuple(MultiTalentLoss(w, batch_dice=True)(outs, tg, case['valid']))
    if cfg['loss'] == 'softmax-torch':          # more than 64 classes: the fused softmax loss refuses them; the reference's, in torch ops on the device
        from oracle import reference_ops as R
        return (R.multiple_output_loss(outs, tg, w, batch_dice=False),)
    return (DC_and_CE_DS_loss(w, batch_dice=False)(outs, tg),)


def set_ds(net, on):
    net.do_ds = on
    if hasattr(net, 'decoder'):
        net.decoder.deep_supervision = on


def hip_step(cfg, net, case, dev, zero_grad=True):
    """forward + loss + backward through the autograd seam -> (logits [cpu], loss values, {name: grad [cpu]})"""
    if zero_grad:
        for p in net.parameters():
            p.grad = None
    out = net(case['x'].to(dev))
    ls = hip_loss(cfg, out, case, dev)
    ls[0].backward()
    torch.cuda.synchronize()
    outs = [out] if torch.is_tensor(out) else list(out)
    logits = [o.detach().float().cpu() for o in outs]
    grads = {n: (p.grad.detach().cpu().clone() if p.grad is not None else None) for n, p in net.named_parameters()}
    return logits, [float(l.detach()) for l in ls], grads


def fresh_net(cfg, dev, precision=None):
    net, _ = EC.build_net(cfg)
    net.train()
    set_ds(net, cfg['ds'])
    eng = net.engine()
    if cfg['streams'] is not None:
        eng.bwdw_streams = cfg['streams']
    if cfg['fuse'] is not None:
        eng.fuse_norm_bwd = cfg['fuse']
    eng.set_precision(cfg['precision'] if precision is None else precision)
    return net


@pytest.mark.parametrize('name', [c['name'] for c in EC.CONFIGS])
def test_engine_path(dev, monkeypatch, name):
    from multitalent_amd import ops
    cfg = EC.CONFIG[name]
    case, sd0, o32, o64 = EC.oracle_pair(cfg)
    mixed = cfg['precision'] != 'fp32'
    try:
        if cfg['wino']:
            ops.set_option('conv_wino', 2)          # the Winograd forms, and with them the fusing forms, also at these sizes
        if mixed:
            ops.set_option('conv_bf16', 2)          # the 16-bit kernels also on these small grids
            ref = hip_step(cfg, fresh_net(cfg, dev, 'fp32'), case, dev)
        net = fresh_net(cfg, dev)
        rec = Recorder(monkeypatch)
        logits, loss, grads = hip_step(cfg, net, case, dev)
        monkeypatch.undo()
    finally:
        ops.set_option('conv_wino', 1)
        ops.set_option('conv_bf16', 1)
        ops.set_mma(0)
    missing = sorted(set(cfg['expects']) - rec.tags)
    print("ENGINE-TAGS %s: %s" % (name, ' '.join(sorted(rec.tags))))
    assert all(g is not None for g in grads.values())
    if not mixed:
        f = EC.figures(grads, o32, o64)
        print("ENGINE-FIG %s: HIP rel. L2 %.2e, fp32 oracle %.2e, cos %.8f, worst tensor %.3f of its bound (%s)" % ((name,) + f))
        assert not missing, "%s: branches that did not run: %s (ran: %s)" % (name, missing, sorted(rec.tags))
        EC.compare(name, logits, loss, grads, o32, o64)
        return
    # mixed precision: the bounds tests/test_mixed_precision_gpu.py states, against the same engine in fp32
    rl, rloss, rg = ref
    ga = torch.cat([grads[n].reshape(-1) for n in grads]).double()
    gb = torch.cat([rg[n].reshape(-1) for n in grads]).double()
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    dl = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(logits, rl))
    print("ENGINE-FIG %s: mixed against fp32 engine: logits %.2e of the largest, loss %.2e, gradient cos %.5f" % (name, dl, abs(loss[0] - rloss[0]), cos))
    assert not missing, "%s: branches that did not run: %s (ran: %s)" % (name, missing, sorted(rec.tags))
    for a, b in zip(logits, rl):
        assert float((a - b).abs().max()) < 3e-2 * float(b.abs().max())
    assert abs(loss[0] - rloss[0]) < 1e-2
    assert cos > 0.99, cos
