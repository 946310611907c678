"""bench.py as the harness of every change runs it: a plain run prints the headline line only (no `roofline`, `cpu_baseline`,
`also`), --steps sets the number of timed steps, and --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'MT_FORCE_REDUCER')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + args, capture_output=True, text=True,
                         timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return lines[0]


@pytest.mark.parametrize("extra, names", [(['--patch', '16', '64', '64', '--batch', '1'], {'loss', 'logits', 'params'}),
                                          (['--workload', 'infer', '--mirror', '0', '--volume', '64', '160', '160', '--patch', '48', '96', '96'],
                                           {'segmentation', 'probabilities'})])
def test_plain_run_headline_only_and_dump(tmp_path, extra, names):
    line = _bench(['--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path)] + extra)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, line
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0
    assert not {'roofline', 'cpu_baseline', 'also'} & set(line), sorted(line)
    files = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(files) == names, sorted(files)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for name, a in files.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), name
    if 'loss' in files:
        assert files['loss'].dtype == np.float64 and abs(float(files['loss'][0]) - line['config']['final_loss']) < 1e-4
