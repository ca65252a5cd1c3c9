"""
CPU tests of the output conversion (float4 -> rgba8 / rgba16 / planar YUV, dithered): the numpy model of tests/output_model.py
against the C oracle (oracle/filters_ref.c: ref_f32_to_rgba, itself held to the reference's pixfmtlib kernels by
tests/test_cpu_golden.py) at every size and format of tests/output_cases.py, and what those cases reach of the 65 536 dither
states.  tests/test_gpu_output.py holds the HIP kernels to the oracle on the same inputs.  Every comparison is exact.
"""
import numpy as np
import pytest

import output_cases as OC
import output_model as OM


@pytest.fixture(scope='module')
def model(built):
    """{(w, h, fmt): (pixels, states after, draws per state)} of the model, computed once for the whole file."""
    out = {}
    for w, h, fmt in OC.cases():
        d, buf = OC.frame(w, h)
        out[w, h, fmt] = OM.convert(d, buf, OC.seeds(), fmt, counts=True)
    return out


@pytest.mark.parametrize('case', OC.cases(), ids=OC.case_id)
def test_model_equals_oracle(model, case):
    """Pixels and all 65 536 states, bit for bit; same shapes and types."""
    pixels, after, _ = model[case]
    ref, ref_after = OC.oracle(*case)
    assert pixels.shape == ref.shape and pixels.dtype == ref.dtype
    assert np.array_equal(pixels, ref), '%d values differ' % int((pixels != ref).sum())
    assert after.shape == (OC.NOUT, 3) and np.array_equal(after, ref_after)


def test_sizes_reach_what_they_are_named_for(built):
    """The size list against its own comments: pixels per state, and the lanes of the four-deep unroll that store."""
    per = {s: OC.served(s[0] * s[1]) for s in OC.SIZES}
    assert per[256, 256].min() == per[256, 256].max() == 1
    assert np.array_equal(per[257, 255], np.r_[np.ones(65535), 0])
    assert (per[256, 257] == 2).sum() == 256 and per[256, 257].max() == 2
    assert per[512, 512].min() == per[512, 512].max() == 4
    for s in ((720, 480), (701, 487)):
        assert set(per[s]) == {5, 6}                          # the second group of four stops after k = 0 or k = 1
    assert set(per[1024, 520]) == {8, 9} and (per[1024, 520] == 9).sum() == 8192
    assert all(s[0] * s[1] < OC.NOUT for s in OC.SIZES[:3]) and OC.STRIDED == OC.SIZES[5:]


@pytest.mark.parametrize('case', OC.cases(OC.STRIDED), ids=OC.case_id)
def test_states_draw_for_more_than_one_pixel(model, case):
    """From 256 x 257 up some states drew for two pixels or more in the same call — counted from the draws, not from the size:
    a state whose draws exceed what one pixel can ask for (4 for rgba, 3 for a YUV pixel).  In 4:2:0 a state of the top-left
    quadrant draws for chroma and, at its next pixel, for luma again."""
    w, h, fmt = case
    _, _, draws = model[case]
    one_pixel = 4 if fmt < OM.YUV444P else 3
    assert int((draws > one_pixel).sum()) > 0
    if fmt == OM.YUV420P10:
        t = np.arange(OC.NOUT)
        chroma_then_luma = ((t % w < w // 2) & (t // w < h // 2) & (t + OC.NOUT < w * h))
        assert int(chroma_then_luma.sum()) > 0


@pytest.mark.parametrize('case', OC.cases(), ids=OC.case_id)
def test_untouched_states(case):
    """States t >= npix serve no pixel: unchanged.  (And every state keeps its multiplier.)"""
    w, h, fmt = case
    _, after = OC.oracle(*case)
    assert np.array_equal(after[w * h:], OC.seeds()[w * h:])
    assert np.array_equal(after[:, 0], OC.seeds()[:, 0])


@pytest.mark.parametrize('case', OC.cases(), ids=OC.case_id)
def test_draw_counts(model, case):
    """A state's draws are as many as its positive components: its MWC stepped that many times, with no look at a pixel
    value, gives the oracle's state.  rgba: the components are the inputs themselves (NaN, -0.0 and -inf are not positive;
    denormals and +inf are).  YUV: the count is the model's own (the components are matrix rows of the inputs)."""
    w, h, fmt = case
    _, ref_after = OC.oracle(*case)
    _, _, draws = model[case]
    if fmt < OM.YUV444P:
        d, buf = OC.frame(w, h)
        crop = buf.reshape(d.ah, d.astride, 4)[OM.GUTTER:OM.GUTTER + h, OM.GUTTER:OM.GUTTER + w]
        with np.errstate(invalid='ignore'):
            positive = (crop > 0).sum(2).reshape(-1)
        mine = np.bincount(np.arange(w * h) % OC.NOUT, weights=positive, minlength=OC.NOUT).astype(np.int64)
        assert np.array_equal(draws, mine)
        if w * h > 33 * 17:
            assert ((crop > 0) & (crop < OC.TINY)).any() and np.isposinf(crop).any()
    assert draws[w * h:].sum() == 0
    assert np.array_equal(OM.advance(OC.seeds(), draws), ref_after)
