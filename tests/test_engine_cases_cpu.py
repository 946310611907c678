"""tests/engine_cases.py without a device: every configuration builds and its oracle runs in fp32 and fp64, the tables are consistent
(the census), the fp32 reference alone stays inside compare() — so a failure on the device is the engine's —, compare() is shown to
reject two wrong gradients, and the torch fact behind Engine._pack's key is pinned."""
import numpy as np
import pytest
import torch

import engine_cases as EC

NAMES = [c['name'] for c in EC.CONFIGS]


def _grads(o):
    return {n: (v.grad.float() if v.grad is not None else torch.zeros_like(v).float()) for n, v in o[0].items()}


@pytest.mark.parametrize('name', NAMES)
def test_config_builds_and_oracle_runs(name):
    cfg = EC.CONFIG[name]
    case, sd0, o32, o64 = EC.oracle_pair(cfg)
    shape = np.array(cfg['shape'])
    total = np.prod(np.array([list(p) for p in cfg['pools']]), 0)
    assert (shape % total == 0).all(), (name, cfg['shape'], total)           # pool / shape divisibility
    assert max(cfg['shape']) <= 32 and cfg['B'] <= 3, name
    assert max(max(v.shape[:2]) for k, v in sd0.items() if v.dim() == 5) <= 144, name       # base <= 72: at most 144 at the bottom
    outs = o64[1]
    tg = case['targets'] if cfg['ds'] else case['targets'][:1]
    assert len(outs) == len(tg)
    for o, t in zip(outs, tg):
        assert tuple(o.shape[2:]) == tuple(t.shape[2:]) and o.shape[0] == t.shape[0] == cfg['B'] and o.shape[1] == cfg['nc']
    for o in (o32, o64):
        assert all(torch.isfinite(l) for l in o[2])
        assert any(v.grad is not None for v in o[0].values())
    assert set(sd0) >= set(o32[0])


def test_census():
    known = set(EC.BRANCHES)
    covered = set()
    for c in EC.CONFIGS + EC.SEQUENCES:
        unknown = set(c['expects']) - known
        assert not unknown, "%s expects tags the table does not know: %s" % (c['name'], sorted(unknown))
        covered |= set(c['expects'])
    assert covered == known, "branches no configuration or sequence expects: %s" % sorted(known - covered)
    assert not (known & set(EC.UNREACHABLE))
    assert all(isinstance(r, str) and len(r) > 20 for r in EC.UNREACHABLE.values())
    assert len(set(NAMES)) == len(NAMES)
    for s in EC.SEQUENCES:
        assert all(n in EC.CONFIG for n in s['on'])
    print("ENGINE-CENSUS %d branches over %d configurations and %d sequences, %d unreachable" % (len(known), len(EC.CONFIGS), len(EC.SEQUENCES),
                                                                                               len(EC.UNREACHABLE)))


@pytest.mark.parametrize('name', sorted({EC.base_key(c): c['name'] for c in EC.CONFIGS}.values()))
def test_fp32_oracle_passes_compare(name):
    cfg = EC.CONFIG[name]
    case, sd0, o32, o64 = EC.oracle_pair(cfg)
    g = _grads(o32)
    print("ENGINE-ORACLE %s: fp32 oracle rel. L2 %.2e, worst tensor %.4f of its bound" % ((name,) + EC.figures(g, o32, o64)[1:4:2]))
    EC.compare(name, o32[1], [float(l) for l in o32[2]], g, o32, o64)


@pytest.mark.parametrize('name', ['p-base10', 'r-base'])
def test_compare_rejects_wrong_gradients(name):
    cfg = EC.CONFIG[name]
    case, sd0, o32, o64 = EC.oracle_pair(cfg)
    loss = [float(l) for l in o32[2]]
    weights = [n for n, v in o32[0].items() if v.dim() == 5 and v.grad is not None and v.shape[2:] == (3, 3, 3)]
    # one weight tensor's gradient scaled by 1.05
    g = _grads(o32)
    g[weights[2]] = g[weights[2]] * 1.05
    with pytest.raises(AssertionError):
        EC.compare(name, o32[1], loss, g, o32, o64)
    # one tensor's gradient replaced by a neighbouring layer's of the same shape
    g = _grads(o32)
    pair = next((a, b) for i, a in enumerate(weights) for b in weights[i + 1:] if g[a].shape == g[b].shape)       # the nearest layer of that shape
    g[pair[0]] = g[pair[1]].clone()
    with pytest.raises(AssertionError):
        EC.compare(name, o32[1], loss, g, o32, o64)


def test_inplace_updates_move_the_parameters_counter_not_the_flat_buffers():
    """The fact Engine._pack's key rests on (plain torch): a parameter re-homed into a flat buffer with `p.data = view` has a version
    counter of its own.  A stock optimizer's step, p.add_() / p.copy_() under no_grad (load_state_dict) change the flat buffer's bytes
    and move p._version, never flat._version; a write through p.data moves neither (that one still needs mark_params_dirty())."""
    flat = torch.zeros(8)
    p = torch.nn.Parameter(torch.ones(4))
    flat[0:4].copy_(p.data)
    p.data = flat[0:4].view(4)
    p.grad = torch.ones(4)

    def moved(f):
        before = (flat._version, p._version, flat.clone())
        f()
        assert not torch.equal(flat, before[2])          # the bytes the engine packs from did change
        return flat._version - before[0], p._version - before[1]

    fv, pv = moved(lambda: torch.optim.SGD([p], lr=1e-2, momentum=0.99, nesterov=True).step())
    assert fv == 0 and pv > 0
    fv, pv = moved(lambda: torch.optim.AdamW([p], lr=1e-2).step())
    assert fv == 0 and pv > 0

    def add():
        with torch.no_grad():
            p.add_(1.0)
    assert moved(add) == (0, 1)

    def copy():
        with torch.no_grad():
            p.copy_(torch.full((4,), 7.0))
    assert moved(copy) == (0, 1)
    assert moved(lambda: p.data.add_(1.0)) == (0, 0)
    assert moved(lambda: flat.add_(1.0)) == (1, 0)
