"""The cases of tests/test_kernel_instances_gpu.py are complete and are what they claim (no GPU): with the built library and fake
pointers, every case resolves to the instance it names and launches, costs at most the cap, and the covered names together with
UNLAUNCHABLE and UNREACHED are exactly the names of the recorded dispatch tables."""
import pytest

import bwdw_dispatch_cases as BC
import conv_dispatch_cases as CC
import instance_cases as IC
import pw_dispatch_cases as PC

CENSUS_N = 20000
# the instance lists the case modules export, per table
INSTANCES = {'bwdd': [i % sd for i in CC.BWDD_INSTANCES for sd in (1, 2)], 'pw': PC.FWD_INSTANCES, 'hb': PC.HB_INSTANCES}


@pytest.fixture(scope='module')
def lib():
    import torch
    from multitalent_amd import _lib
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != 256:
            pytest.skip("the dispatch tables are recorded for 256 compute units; this device has %d" % cus)
    return _lib.load()


def _ask(lib, table, major, minor):
    """(name, launches) of a row with the table's fake pointers"""
    t = IC.TABLES[table][0]
    got = t.query(lib, *t.problem(major, minor))
    cols = {k: [v] for (k, _), v in zip(t.COLUMNS, got[1:])}
    return got[0], IC.launches(table, cols, 0, major, minor, got[0])


def _table_names(table):
    return {n for n in IC.recorded(table)[1] if not n.startswith('<rc')}


@pytest.mark.parametrize('table', IC.ORDER)
def test_every_case_is_the_instance_it_claims_and_launches(lib, table):
    cases = IC.cases(table)
    assert cases
    for _, major, minor, name in cases:
        assert _ask(lib, table, major, minor) == (name, True), (major, minor, name)
        assert IC.valid_addresses(table, major, minor), (major, minor)
        assert IC.cost(table, major, minor) <= IC.COST_CAP, (major, minor, IC.cost(table, major, minor))
    assert len({IC.case_id(c) for c in cases}) == len(cases)


@pytest.mark.parametrize('table', IC.ORDER)
def test_every_instance_is_run_or_listed(table):
    names = _table_names(table)
    covered = {c[3] for c in IC.cases(table)}
    unl, unr = set(IC.UNLAUNCHABLE[table]), set(IC.UNREACHED[table])
    assert not (covered & unl) and not (covered & unr) and not (unl & unr)
    assert covered | unl | unr == names, (sorted(names - covered - unl - unr), sorted((covered | unl | unr) - names))
    assert set(INSTANCES.get(table, [])) <= names


@pytest.mark.parametrize('table', IC.ORDER)
def test_unlaunchable_names_launch_on_no_row_of_the_table(table):
    rows, names, cols = IC.recorded(table)
    for i, n in enumerate(names):
        assert n not in IC.UNLAUNCHABLE[table] or not IC.launches(table, cols, i, rows[i][0], rows[i][1], n), (n, rows[i])


@pytest.mark.parametrize('table', IC.ORDER)
def test_unreached_names_are_few_launchable_and_above_the_cap(lib, table):
    assert len(IC.UNREACHED[table]) <= 2
    rows, names, cols = IC.recorded(table)
    for name, (major, minor, macs) in IC.UNREACHED[table].items():
        assert _ask(lib, table, major, minor) == (name, True)
        assert IC.cost(table, major, minor) == macs > IC.COST_CAP
        # the smallest launchable problem the recorded table knows
        assert macs == min(IC.cost(table, *rows[i]) for i, n in enumerate(names)
                           if n == name and IC.launches(table, cols, i, rows[i][0], rows[i][1], n) and IC.valid_addresses(table, *rows[i]))


@pytest.mark.parametrize('table', IC.ORDER)
def test_name_census_is_closed(lib, table):
    """Over a fixed, hash-drawn sample of the FULL axis product no kernel name appears that the recorded table lacks."""
    t = IC.TABLES[table][0]
    have = set(IC.recorded(table)[1])
    new = {}
    for major, minor in BC.census_rows(t, CENSUS_N):
        new.setdefault(t.query(lib, *t.problem(major, minor))[0], (major, minor))
    assert set(new) <= have, {n: r for n, r in new.items() if n not in have}
