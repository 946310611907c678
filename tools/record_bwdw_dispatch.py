#!/usr/bin/env python
"""Record the backward-weight dispatch table behind tests/test_bwdw_dispatch_cpu.py.

For every problem of tests/bwdw_dispatch_cases.py: the kernel name mt_conv3d_bwd_weight_kernel_name reports (as an index into a
name list), mt_conv3d_bwd_weight_workspace and mt_conv3d_bwd_weight_io_supported -> tests/golden/bwdw_dispatch.npz.  The queries
read descriptors only, so this runs without a GPU; the table is for 256 compute units (the library's answer without a device, and
the MI355X's count).  Re-record only when the dispatch POLICY changes on purpose: the diff of the table is then the review record.

    python tools/record_bwdw_dispatch.py [--lib path/to/libmtseg_hip.so] [--census N]

--census N draws N rows uniformly from the FULL product of the axes and lists kernel names the thinned table does not contain
(rows to add to bwdw_dispatch_cases.EXTRA); nothing is written.
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
from multitalent_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bwdw_dispatch.npz')


def census(lib, n, have):
    axes = BC.MAJOR + BC.MINOR
    total = 1
    for ax in axes:
        total *= len(ax)
    missing = {}
    for i in range(n):
        pick = BC._pick(axes, (BC._mix(i) * 0x100000000 + BC._mix(i + 0x9e3779b9)) % total)
        major, minor = pick[:len(BC.MAJOR)], pick[len(BC.MAJOR):]
        name = BC.query(lib, *BC.problem(major, minor))[0]
        if name not in have:
            missing.setdefault(name, (major, minor))
    print("%d of %d rows of the full product sampled; %d kernel names missing from the table" % (n, total, len(missing)))
    for name, row in sorted(missing.items()):
        print("    %r,    # %s" % (row, name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', help='shared library to ask (default: the package\'s)')
    ap.add_argument('--census', type=int, default=0)
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        sys.exit("the table is recorded for 256 compute units; hide this device (HIP_VISIBLE_DEVICES=) to record it")
    lib = _lib.load()
    names, ws, io = BC.query_all(lib)
    if a.census:
        census(lib, a.census, set(names))
        return
    name_list = sorted(set(names))
    index = {n: i for i, n in enumerate(name_list)}
    np.savez_compressed(GOLDEN, names=np.array(name_list), name=np.array([index[n] for n in names], dtype=np.int16),
                        workspace=np.array(ws, dtype=np.int64), io_supported=np.array(io, dtype=np.uint8))
    fams = collections.Counter(BC.family(n) for n in names)
    print("%d rows, %d kernel names, %d bytes -> %s" % (len(names), len(name_list), os.path.getsize(GOLDEN), GOLDEN))
    print("rows per family: " + ", ".join("%s %d" % kv for kv in sorted(fams.items(), key=lambda kv: str(kv[0]))))


if __name__ == '__main__':
    main()
