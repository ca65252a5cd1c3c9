"""
CPU side of the one-direction tests of the bilateral DE (tests/de_dir_cases.py, tests/de_dir_model.py; the device side is
tests/test_gpu_de_dir.py): the float64 model against the float32 oracle on every case, the bar B of every class under its cap,
the kinds of tile every frame reaches, the lone bins' supports and the margin of the shift test.  Run with -s for the tables.

B of a class (direction family x input kind x parameter set) = max(4 e_oracle + T_pow, 4 * 2^-24), e_oracle = the oracle's worst
|x - m| / (|m| + 2^-10 M_c) against the model over the class's directions and frames, T_pow derived (de_dir_cases.t_pow).  A
class whose B exceeds 1e-4 is ill-conditioned and has to be replaced by another input, not given a wider bar.
Measured (x86-64 glibc): e_oracle 7.2e-7 .. 1.5e-5 (largest: integer steps, sparse, dpow 0), T_pow 2.4e-7 (dpow 0) and 1.3e-5
(dpow 0.8, density 64), B 3.1e-6 .. 6.7e-5; lone bins e_oracle 3.6e-7, T_pow 1.1e-7, B 1.6e-6.
"""
import numpy as np
import pytest

import de_dir_cases as Cs
import de_dir_model as M
from common import O

CLASSES = [(f, k, p) for f in Cs.FAMILIES for k in Cs.KINDS for p in Cs.PSETS]


def test_geometry_restatements_agree():
    """The cases' integer tap offsets are the model's rint offsets, the restated de_reach gives the halos de.hip's header lists,
    and the model's blur coefficients are the oracle's."""
    for P in range(8):
        assert [Cs.tap(P, r) for r in range(-16, 17)] == M.tap_offsets(P, range(-16, 17)), P
        assert Cs.reach(P) == Cs.HALO[P], (P, Cs.reach(P))
    assert np.abs(M.gauss7() - O.gauss_coefs(1)).max() <= 2.0 ** -24


def test_frames_reach_their_tile_layouts():
    """Border and interior tiles per frame and direction, from the restated `border` predicate: 1 x 1 and 33 x 17 are all
    border with one / two rows of tiles, 8 x 300 has one tile column in direction 0, 300 x 8 one tile row in the others, and
    200 x 120 has both kinds of tile in directions 0, 1, 5 and 7 (140 tiles in direction 1)."""
    for size in Cs.FRAMES + [Cs.SHIFT_FRAME]:
        for P in range(8):
            nx, ny, nb, ni = Cs.check_frame(size, P)
            print('%4d x %-4d direction %d: %3d x %-3d tiles, %4d border, %4d interior' % (size + (P, nx, ny, nb, ni)))
    none = [P for P in range(8) if Cs.tile_kinds(P, *Cs.padded((200, 120)))[1] == 0]
    print('200 x 120 has no interior tile in directions %s (their interior form: the shift test)' % (none or 'none'))
    assert not set(none) & {0, 1, 5, 7}
    for P in range(8):
        assert Cs.tile_kinds(P, *Cs.padded(Cs.SHIFT_FRAME))[1] > 0


@pytest.mark.parametrize('fam,kind,pset', CLASSES)
def test_model_against_oracle_and_bound(fam, kind, pset):
    """The oracle pass stays within e_oracle of the model on every direction and frame of the class, and the class's B stays
    under the cap."""
    B, e, t = Cs.bound(fam, kind, pset)
    print('%-10s %-6s %-10s e_oracle %.3g  T_pow %.3g  B %.3g' % (fam, kind, pset, e, t, B))
    for P in Cs.FAMILIES[fam]:
        for size in Cs.FRAMES:
            want = Cs.case_a(P, size, kind, pset)[1]
            assert np.isfinite(want[..., 3]).all() and (want[..., 3] >= 0).all()
            assert np.isfinite(want).mean() > 0.5, 'most colours are pinned'
    assert Cs.FLOOR <= B <= Cs.CAP, (B, e, t)


def test_first_direction_yuv_case_clamps():
    """Section E's in_mode 2 inputs hold live pixels whose RGB clamps at 0, and the model is fed the clamped picture."""
    for kind in Cs.KINDS:
        for size in ((33, 17), (200, 120)):
            yuv = Cs.accumulator(kind, size, yuv=True)
            dev_in, raw64 = Cs.device_forms(0, yuv, in_mode=2)
            u, v = yuv[..., 1] - 0.5 * yuv[..., 3], yuv[..., 2] - 0.5 * yuv[..., 3]
            neg = (yuv[..., 3] > 0) & ((yuv[..., 0] + 1.402 * v < 0) | (yuv[..., 0] + 1.772 * u < 0))
            assert neg.sum() >= 10 and (raw64[..., :3] >= 0).all() and (raw64[neg][:, :3] == 0).any(), (kind, size, neg.sum())
            assert dev_in is yuv
            B = Cs.bound('horizontal', kind, 'default')[0]
            e = Cs.case_a(0, size, kind, 'default', in_mode=2)[2]
            print('in_mode 2 %-6s %3d x %-3d: %d clamped pixels, e_oracle %.3g (B %.3g)' % ((kind,) + size + (neg.sum(), e, B)))
            assert 4 * e <= B


@pytest.mark.parametrize('P', range(8))
def test_lone_bins_reach_their_cases(P):
    """Lone bins: the oracle's output is nonzero only on the support the geometry gives (asserted in de_dir_cases.lone_case),
    interior bins have exactly 31 support pixels with model densities far from flush-to-zero, the positions sweep every column
    and row of the direction's tile, and the class's B stays under the cap."""
    smallest = {}
    for size in Cs.FRAMES:
        for sstd in Cs.LONE_SSTD:
            smallest[sstd] = min(smallest.get(sstd, 1.0), Cs.check_lone(P, size, sstd)[1])
            for dev_in, sup, want, pts in Cs.lone_case(P, size, sstd)[0]:
                assert all(sup[p] for p in pts) and np.isfinite(want[:, 3]).all()
    B, e, t = Cs.bound(Cs.family(P), 'lone', None)
    print('direction %d lone bins: smallest interior model density %.3g (sstd 24), %.3g (sstd 6); e_oracle %.3g T_pow %.3g B %.3g' % (
        P, smallest[24.0], smallest[6.0], e, t, B))
    assert Cs.FLOOR <= B <= Cs.CAP


def test_shift_margin():
    """The shift test's rectangle lies in interior tiles under every shift; the margin follows from HU, HV and the shear."""
    worst = [0, 0]
    for P in range(8):
        my, mx = Cs.check_shift(P)
        n = len(Cs.shifts(P))
        TW, TH = Cs.tile_shape(P)
        assert n >= TW - 1 + TH - 1 + min(TW * TH, 64) - (TW + TH)
        print('direction %d: interior beyond %2d rows, %3d columns; %d shifts' % (P, my, mx, n))
        worst = [max(worst[0], my), max(worst[1], mx)]
    assert worst[0] <= 96 and worst[1] <= 192, worst
    for kind in Cs.KINDS:
        pic = Cs.shift_picture(kind)
        assert pic.shape[:2] == Cs.PICTURE


def test_model_converters_and_ratio():
    """to_normalised / to_raw invert each other on float32 inputs, dead pixels have colour 0, and `ratio` counts a non-finite
    value against a finite model value as a failure and skips unpinned (NaN) model values."""
    raw = np.float32([[[3.0, 1.5, 0.75, 3.0], [0.0, 0.0, 0.0, 0.0], [1e-3, 2e-3, 0.0, 7.0]]])
    N = M.to_normalised(raw)
    assert np.array_equal(N[0, 0], [1.0, 0.5, 0.25, 3.0]) and not N[0, 1].any()
    assert np.allclose(M.to_raw(N), raw, rtol=1e-15, atol=0)
    m = np.array([[1.0, 2.0, np.nan, 4.0], [0.5, 0.0, 1.0, 2.0]])
    x = m.copy(); x[0, 2] = 7.0
    assert M.ratio(x, m)[0] == 0.0
    x[1, 1] = np.nan
    assert M.ratio(x, m)[0] == np.inf
    x[1, 1] = 2.0 ** -10 * 2.0
    assert abs(M.ratio(x, m)[0] - 1.0) < 1e-12
    out, S = M.bilateral_pass(np.zeros((8, 8, 4)), 4, (6.0, 0.05, 1.5, 0.8, 4.0))
    assert not out.any() and not S.any() and not M.normalised_out(out, S).any()
