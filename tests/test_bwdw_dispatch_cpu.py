"""Backward-weight dispatch is pinned row by row (no GPU): for every problem of bwdw_dispatch_cases the kernel name, the workspace
query and io_supported equal tests/golden/bwdw_dispatch.npz (tools/record_dispatch.py --table bwdw).  A change of dispatch policy shows up
as a re-recorded table."""
import os

import numpy as np
import pytest

import bwdw_dispatch_cases as BC
from bwdw_dispatch_cases import _first_diff

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bwdw_dispatch.npz')


@pytest.fixture(scope='module')
def table():
    import torch
    from multitalent_amd import _lib
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != 256:
            pytest.skip("the dispatch table is recorded for 256 compute units; this device has %d" % cus)
    gold = np.load(GOLDEN)
    names, ws, io = BC.query_all(_lib.load())
    return gold, names, ws, io


def test_kernel_names_match_the_recorded_table(table):
    gold, names, _, _ = table
    want = [str(n) for n in gold['names'][gold['name']]]
    assert len(names) == len(want)
    assert _first_diff(BC.rows(), names, want) is None, _first_diff(BC.rows(), names, want)


def test_workspace_matches_the_recorded_table(table):
    gold, _, ws, _ = table
    assert len(ws) == len(gold['workspace'])
    assert _first_diff(BC.rows(), np.array(ws, dtype=np.int64), gold['workspace']) is None, _first_diff(BC.rows(), np.array(ws, dtype=np.int64), gold['workspace'])


def test_io_supported_matches_the_recorded_table(table):
    gold, _, _, io = table
    assert len(io) == len(gold['io_supported'])
    assert _first_diff(BC.rows(), np.array(io, dtype=np.uint8), gold['io_supported']) is None, _first_diff(BC.rows(), np.array(io, dtype=np.uint8), gold['io_supported'])


def test_every_family_occurs(table):
    gold = table[0]
    fams = {BC.family(str(n)) for n in gold['names']}
    assert None not in fams, [str(n) for n in gold['names'] if BC.family(str(n)) is None]
    assert fams == set(BC.FAMILIES), set(BC.FAMILIES) - fams
    assert {'conv_bwdw_wino_kernel<2>', 'conv_bwdw_wino_kernel<2, KD = 1>'} <= {str(n) for n in gold['names']}
