#!/usr/bin/env python
"""Record a dispatch table: the golden file behind tests/test_bwdw_dispatch_cpu.py, test_conv_dispatch_cpu.py or test_pw_dispatch_cpu.py.

    python tools/record_dispatch.py --table bwdw|conv|pw [--lib path/to/libmtseg_hip.so] [--out file.npz] [--census N]

bwdw: tests/bwdw_dispatch_cases.py -> tests/golden/bwdw_dispatch.npz (mt_conv3d_bwd_weight: kernel name, workspace, io_supported).
conv: tests/conv_dispatch_cases.py -> tests/golden/conv_dispatch.npz, two sets of rows: FWD (mt_conv3d_fwd: kernel name, ck, pack layout,
statistics partials, io_supported, bwd_stats_supported) and BWDD (mt_conv3d_bwd_data_strided: kernel name, supported, pack layout,
io_supported; keys prefixed 'bwdd_').
pw: tests/pw_dispatch_cases.py -> tests/golden/pw_dispatch.npz, two sets of rows: FWD (mt_pointwise_fwd: return code, kernel instance, grid
and store form, pack layout, io_supported, statistics partials) and HB (mt_head_bwd: return code, kernel instance, dbias_done, supported,
io_supported, workspace; keys prefixed 'hb_').  Kernel names are stored as indices into a name list.

The queries read descriptors only, so this runs without a GPU; the tables are for 256 compute units (the library's answer without a
device, and the MI355X's count).  Re-record only when the dispatch POLICY changes on purpose: the diff of the table is then the review
record.

--census N draws N rows uniformly from the FULL product of each table's axes and lists kernel names the thinned table does not contain
(rows to add to the table's EXTRA); nothing is written.
"""
import argparse
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bwdw_dispatch_cases as BC  # noqa: E402
import conv_dispatch_cases as CC  # noqa: E402
import pw_dispatch_cases as PC  # noqa: E402
from multitalent_amd import _lib  # noqa: E402

TABLES = {'bwdw': ('bwdw_dispatch.npz', [BC]), 'conv': ('conv_dispatch.npz', [CC.FWD, CC.BWDD]),
          'pw': ('pw_dispatch.npz', [PC.FWD, PC.HB])}


def census(lib, t, n, have):
    total = 1
    for ax in t.MAJOR + t.MINOR:
        total *= len(ax)
    missing = {}
    for major, minor in BC.census_rows(t, n):
        name = t.query(lib, *t.problem(major, minor))[0]
        if name not in have:
            missing.setdefault(name, (major, minor))
    print("%d of %d rows of the full product sampled; %d kernel names missing from the table" % (n, total, len(missing)))
    for name, row in sorted(missing.items()):
        print("    %r,    # %s" % (row, name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--table', required=True, choices=sorted(TABLES))
    ap.add_argument('--lib', help='shared library to ask (default: the package\'s)')
    ap.add_argument('--out', help='file to write (default: the table\'s golden file)')
    ap.add_argument('--census', type=int, default=0)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        sys.exit("the table is recorded for 256 compute units; hide this device (HIP_VISIBLE_DEVICES=) to record it")
    lib = _lib.load()
    fname, tables = TABLES[a.table]
    out = a.out or os.path.join(ROOT, 'tests', 'golden', fname)
    arrays = {}
    for t in tables:
        names, cols = BC.ask(lib, t)
        if a.census:
            census(lib, t, a.census, set(names))
            continue
        name_list = sorted(set(names))
        index = {n: i for i, n in enumerate(name_list)}
        arrays[t.PREFIX + 'names'] = np.array(name_list)
        arrays[t.PREFIX + 'name'] = np.array([index[n] for n in names], dtype=np.int16)
        for k, dt in t.COLUMNS:
            arrays[t.PREFIX + k] = np.array(cols[k], dtype=dt)
        fams = collections.Counter(t.family(n) for n in names)
        print("%s%d rows, %d kernel names" % (t.PREFIX and t.PREFIX + ': ', len(names), len(name_list)))
        print("rows per family: " + ", ".join("%s %d" % kv for kv in sorted(fams.items(), key=lambda kv: str(kv[0]))))
    if arrays:
        np.savez_compressed(out, **arrays)
        print("%d bytes -> %s" % (os.path.getsize(out), out))


if __name__ == '__main__':
    main()
