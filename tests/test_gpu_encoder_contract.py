"""
What every device encoder's entry points promise (tests/encoder_contract.py), once per clause and row: capacity, a pageable host
destination, a device destination at an odd address, refusals, the whole path, and the timing slot.  What is an encoder's own —
its files against its model, its tile, segment and restart edges — is in its test_gpu_<format>.py.
"""
import pytest

import encoder_contract as EC

pytestmark = pytest.mark.gpu
mgr = EC.mgr_fixture()
rows = pytest.mark.parametrize('row', EC.ROWS, ids=repr)


@rows
def test_capacity(mgr, row):
    EC.check_capacity(mgr, row)


@rows
def test_pageable(mgr, row):
    EC.check_pageable(mgr, row)


@rows
def test_device_destination(mgr, row):
    EC.check_device_destination(mgr, row)


@rows
def test_refusals(mgr, row):
    EC.check_refusals(mgr, row)


@pytest.mark.parametrize('row', [r for r in EC.ROWS if r.whole], ids=repr)
def test_whole_path(mgr, row):
    EC.check_whole_path(mgr, row)


@rows
def test_timed(mgr, row):
    EC.check_timed(mgr, row)
