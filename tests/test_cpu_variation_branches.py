"""
The fixed variation branch cases (tests/variation_branch_cases.py) do what they say, judged on the CPU with numpy predicates on the
inputs and the oracle alone: every named branch of every case is reached by at least 32 of its 1024 points, the oracle's result is
finite for at least 90 % of them, and at most 1.5 % of them have an oracle neighbourhood that spreads beyond the plain tolerance —
the cap that tests/test_gpu_variations.py puts on its neighbourhood clause, here a condition that the case meets before any device
is asked.
"""
import numpy as np
import pytest

import variation_branch_cases as B
from cuburn_amd.genome import variations as V


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=[c['id'] for c in B.CASES])
def test_case_reaches_its_branches(built, index):
    c = B.CASES[index]
    view = B.oracle_view(c, index)
    seen = view['seen']
    assert seen.w == np.float32(c['weight']) and int(seen.xf[16:17].astype(np.float32).view(np.int32)[0]) == V.var_ids[c['var']]
    for label, pred in c['branches'].items():
        n = int(np.asarray(pred(seen)).sum())
        assert n >= 32, (c['id'], label, n)
    assert np.isfinite(view['ref']).all(1).mean() >= 0.9, c['id']
    assert view['spread_share'] <= 0.015, (c['id'], view['spread_share'])


def test_the_cases_cover_what_they_were_promoted_for():
    ids = [c['id'] for c in B.CASES]
    assert len(set(ids)) == len(ids)
    have = set(c['var'] for c in B.CASES)
    for var in ('disc2', 'rectangles', 'loonie', 'lazysusan', 'whorl', 'bipolar', 'modulus', 'oscope', 'fan', 'fan2', 'rings',
                'rings2', 'julian', 'juliascope', 'cpow', 'ngon', 'perspective', 'splits', 'bent', 'bent2', 'separation', 'boarders',
                'cell', 'exponential', 'sin', 'cos', 'tan', 'sec', 'csc', 'cot', 'sinh', 'cosh', 'tanh', 'sech', 'csch', 'coth', 'cosine'):
        assert var in have, var
    assert all(c['span'] in (0.3, 1.5, 5.0) for c in B.CASES)
    assert any(c['weight'] < 0 for c in B.CASES)
