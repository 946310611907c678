"""Pointwise and head-backward dispatch are pinned row by row (no GPU): for every problem of pw_dispatch_cases the kernel instance, the
return code, the launch shape and every query over the decision equal tests/golden/pw_dispatch.npz (tools/record_dispatch.py --table pw).
A change of dispatch policy shows up as a re-recorded table.  Nothing in these decisions reads the compute-unit count (see
pw_dispatch_cases), so there is no device to skip on."""
import os

import numpy as np
import pytest

import pw_dispatch_cases as PC
from bwdw_dispatch_cases import _first_diff, ask

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pw_dispatch.npz')
TABLES = (PC.FWD, PC.HB)
COLUMNS = [(t, k) for t in TABLES for k, _ in t.COLUMNS]


@pytest.fixture(scope='module')
def tables():
    from multitalent_amd import _lib
    lib = _lib.load()
    return np.load(GOLDEN), {t.PREFIX: (t.rows(),) + ask(lib, t) for t in TABLES}


def _recorded(gold, t):
    return [str(n) for n in gold[t.PREFIX + 'names'][gold[t.PREFIX + 'name']]]


@pytest.mark.parametrize('t', TABLES, ids=['fwd', 'hb'])
def test_kernel_names_match_the_recorded_table(tables, t):
    gold, got = tables
    rows, names, _ = got[t.PREFIX]
    want = _recorded(gold, t)
    assert len(names) == len(want)
    assert _first_diff(rows, names, want) is None, _first_diff(rows, names, want)


@pytest.mark.parametrize('t,key', COLUMNS, ids=[t.PREFIX + k for t, k in COLUMNS])
def test_query_matches_the_recorded_table(tables, t, key):
    gold, got = tables
    rows, _, cols = got[t.PREFIX]
    want = gold[t.PREFIX + key]
    assert len(cols[key]) == len(want)
    assert _first_diff(rows, np.array(cols[key], dtype=want.dtype), want) is None, _first_diff(rows, np.array(cols[key], dtype=want.dtype), want)


def test_every_family_occurs(tables):
    gold = tables[0]
    rows, names = PC.FWD.rows(), _recorded(gold, PC.FWD)
    # all three kernels, every instance the launcher can pick (both M16 forms among them) and a refusal
    assert {PC.FWD.family(n) for n in names if not n.startswith('<rc')} == set(PC.FWD.FAMILIES)
    assert set(PC.FWD_INSTANCES) | {'<rc -1>'} == set(names), set(PC.FWD_INSTANCES) ^ set(names)
    assert {int(w) for w in gold['wide']} == {0, 1, 2}
    # eight taps: two workgroups of four without statistics (z = 2), pw_fast_kernel<8, ...> with them
    eight = [(n, int(z), minor[7]) for (major, minor), n, z, rc in zip(rows, names, gold['grid_z'], gold['rc']) if major[0] == PC.G_T8 and rc == 0]
    assert eight and all(n.startswith('pw_fast_kernel<8, ') and z == 1 if stats else n.startswith('pw_fast_kernel<4, ') and z == 2
                         for n, z, stats in eight)
    assert {int(z) for z in gold['grid_z'][gold['rc'] == 0]} == {1, 2}
    # a 33..64-channel head with Vb % 32 != 0 falls back to two channel tiles of pw_fast_kernel<1, ...>
    i = rows.index(PC.FWD_EXTRA[-1])
    assert names[i] == 'pw_fast_kernel<1, 0, 0, false>' and int(gold['grid_y'][i]) == 2
    # Cin = 1040 exceeds the LDS copy of scale / shift: refused
    assert all(rc != 0 for (major, _), rc in zip(rows, gold['rc']) if major[1] == 1040)
    # head backward: every instance, and the refusal
    hnames = _recorded(gold, PC.HB)
    assert set(PC.HB_INSTANCES) | {'<rc -1>'} == set(hnames), set(PC.HB_INSTANCES) ^ set(hnames)
    assert {int(d) for d in gold['hb_dbias_done'][gold['hb_rc'] == 0]} == {0, 1}
