"""Forward and strided backward-data dispatch are pinned row by row (no GPU): for every problem of conv_dispatch_cases the kernel name
and every query over the dispatch decision equal tests/golden/conv_dispatch.npz (tools/record_dispatch.py --table conv).  A change of
dispatch policy shows up as a re-recorded table."""
import os

import numpy as np
import pytest

import conv_dispatch_cases as CC
from bwdw_dispatch_cases import _first_diff

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_dispatch.npz')
COLUMNS = [(t, k) for t in (CC.FWD, CC.BWDD) for k, _ in t.COLUMNS]


@pytest.fixture(scope='module')
def tables():
    import torch
    from multitalent_amd import _lib
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != 256:
            pytest.skip("the dispatch table is recorded for 256 compute units; this device has %d" % cus)
    lib = _lib.load()
    return np.load(GOLDEN), {t.PREFIX: (t.rows(),) + CC.ask(lib, t) for t in (CC.FWD, CC.BWDD)}


@pytest.mark.parametrize('t', [CC.FWD, CC.BWDD], ids=['fwd', 'bwdd'])
def test_kernel_names_match_the_recorded_table(tables, t):
    gold, got = tables
    rows, names, _ = got[t.PREFIX]
    want = [str(n) for n in gold[t.PREFIX + 'names'][gold[t.PREFIX + 'name']]]
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
    names = {str(n) for n in gold['names']}
    fams = {CC.FWD.family(n) for n in names}
    assert None not in fams, [n for n in names if CC.FWD.family(n) is None]
    assert fams == set(CC.FWD.FAMILIES), set(CC.FWD.FAMILIES) - fams
    # the KD = 1 forms of fast, bf16 and x16; the two-tile gather; both forms of the generic kernel
    assert {'conv_fast_kernel<32, 4, 2, 2, 1>', 'conv_bf16_kernel<32, 4, 4, 4, 1, 4, 1, 2, 2, 2>', 'conv_x16_kernel<1, 2>',
            'conv_gather_kernel<4, 0, 0, false, 2>', 'conv_fwd_kernel<8, 2, 2, 16, true>', 'conv_fwd_kernel<8, 2, 2, 16, false>'} <= names
    # the pair of planes around the packed-offset limit of the persistent Winograd kernel
    rows = CC.FWD.rows()
    at = {(major[2][1:], minor[6]): str(gold['names'][gold['name'][i]]) for i, (major, minor) in enumerate(rows) if major[2][0] == 4}
    assert at[(400, 522), False] == 'conv_wino8p_kernel' and at[(400, 522), True] == 'conv_wino8pb_kernel'
    assert not at[(400, 524), False].startswith('conv_wino') and not at[(400, 524), True].startswith('conv_wino')
    # strided backward-data: every instance the launcher can pick, and the refusal
    bnames = {str(n) for n in gold['bwdd_names']}
    assert {i % sd for i in CC.BWDD_INSTANCES for sd in (1, 2)} | {'<rc -1>'} == bnames, bnames
