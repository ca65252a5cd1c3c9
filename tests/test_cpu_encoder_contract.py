"""
tests/encoder_contract.py against the library's prototype table, without a device: every fl_X_encode* has a row (or a reason),
every row's names exist, its refused calls are calls of its prototype that differ from the good one, and its overflow caps
really overflow without being refused — by the model alone.
"""
import re

import pytest

from cuburn_amd import _lib
import encoder_contract as EC

rows = pytest.mark.parametrize('row', EC.ROWS, ids=repr)


def test_every_encode_entry_point_has_a_row():
    entries = [n for n in _lib.EXPORTS if re.match(r'fl_\w+_encode(_\w)?$', n)]
    assert len(entries) >= 10, entries
    covered = set(r.encode for r in EC.ROWS)
    missing = [n for n in entries if n not in covered and n not in EC.EXEMPT]
    assert not missing, 'no row of encoder_contract.ROWS (and no reason in EXEMPT) for %s' % ', '.join(missing)
    assert not set(EC.EXEMPT) & covered and set(EC.EXEMPT) <= set(entries) and all(EC.EXEMPT.values())
    assert len(set(r.name for r in EC.ROWS)) == len(EC.ROWS)


@rows
def test_names_and_arity(row):
    sigs = _lib._SIGS
    for name in (row.encode, row.output, row.bound) + tuple(f[0] for f in row.facts):
        assert name in sigs, '%s: %s is not in the prototype table' % (row.name, name)
    for clause in EC.CLAUSES:
        for name in EC.sources_of(row, clause):
            arr, mid = row.source(name, row.model_param(None) if row.probe else None)
            w, h = EC.dims(row, arr)
            good = (w, h, 1) + tuple(mid) + (2, 0, 1 << 20)
            assert 1 + len(good) == len(sigs[row.encode][1]), '%s: %s takes %d arguments, the good call has %d' % (row.name, row.encode, len(sigs[row.encode][1]), 1 + len(good))
            assert 2 + len(row.bound_args(mid)) == len(sigs[row.bound][1]), '%s: %s' % (row.name, row.bound)
            calls = EC.refused_calls(row, w, h, 1, mid, 2, 1 << 20)
            assert len(calls) == len(row.refused) + 3
            for edit, code, enc, out in calls:
                assert len(enc) == len(good) and enc != good, '%s: refused %r is the good call' % (row.name, edit)
                assert code in (EC.INVAL, EC.UNSUPPORTED)
                if out is not None:
                    assert 1 + len(out) == len(sigs[row.output][1]), '%s: %s takes %d arguments, %r' % (row.name, row.output, len(sigs[row.output][1]), out)
                    assert out != (w, h) + tuple(mid[row.lead:]) + (2, 0, 1 << 20), '%s: refused %r is a good call of %s' % (row.name, edit, row.output)
    for fmt, w, h, mids in row.whole:
        assert fmt in EC.PLAIN and fmt in _lib.OUT and all(3 + len(mid[row.lead:]) + 3 == len(sigs[row.output][1]) and 4 + len(mid) + 3 == len(sigs[row.encode][1]) for mid in mids), (row.name, fmt)


@rows
def test_overflow_caps_overflow_and_are_not_refused(row):
    for name in EC.sources_of(row, 'capacity'):
        param = row.model_param(None) if row.probe else None
        arr, mid = row.source(name, param)
        w, h = EC.dims(row, arr)
        need = len(row.model(arr, mid, row.model_param(mid)))
        lo = row.min_cap(w, h, mid)
        assert lo < 16 + need, '%s: %r: min_cap %d holds the whole file of %d bytes' % (row.name, name, lo, need)
        caps = EC.overflow_caps(row, need, w, h, mid)
        assert len(caps) >= 2 and all(lo <= cap < 16 + need for cap in caps), '%s: %r: caps %r, min_cap %d, the file %d' % (row.name, name, caps, lo, need)
