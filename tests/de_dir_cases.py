"""
The cases of tests/test_cpu_de_dir.py (no GPU) and tests/test_gpu_de_dir.py: inputs and parameters for ONE direction of the
bilateral DE (csrc/de.hip k_de_dir through fl_debug_de_dir), each with a check that it still reaches the part of the kernel it
is named for, the float64 model's results (tests/de_dir_model.py) and the bars B, kept once per session.

The geometry below restates csrc/de.hip (de_shear, de_reach, DeGeo's tile shapes, the kernel's `border` predicate) so that the
cases can say which tiles of a frame take the nested form with frame tables and which the two-phase form.
"""
import functools
import math

import numpy as np

from common import O
import de_dir_model as M
from accum_inputs import synth_accum, sparse_accum

# ---------------------------------------------------------------------------------------------- geometry (csrc/de.hip)
K = (0, 0, 2, -2, 4, -1, -4, 1)                    # x step per two rows of a sheared tile
NUM = ((2, 0), (0, 2), (2, 2), (-2, 2), (2, 1), (-1, 2), (2, -1), (1, 2))      # twice the slopes
HALO = ((0, 24), (24, 0), (24, 0), (24, 0), (13, 2), (24, 1), (13, 2), (24, 1))    # HU, HV as the kernel's header states them
FAMILIES = {'horizontal': (0,), 'integer': (1, 2, 3), 'half': (4, 5, 6, 7)}


def family(P):
    return next(f for f, ps in FAMILIES.items() if P in ps)


def tile_shape(P):
    return (64, 4) if P == 0 else (8, 32)           # TW, TH


def rne_half(v):
    return v // 2 if v % 2 == 0 else ((v - 1) // 2 if (v - 1) // 2 % 2 == 0 else (v + 1) // 2)


def tap(P, r):
    return rne_half(NUM[P][0] * r), rne_half(NUM[P][1] * r)


def shear(P, j):
    return (j * K[P]) // 2


def dv(P, par, dx, dy):
    return dx - (shear(P, par + dy) - shear(P, par))


def reach(P):
    """de_reach(P, true): the largest row / column displacement (sheared coordinates) of a staged value a tile pixel needs."""
    hu = hv = 0
    for par in (0, 1):
        for r in range(-16, 17):
            for i in range(-3, 4):
                for j in range(-3, 4):
                    if abs(r) == 16 and (i or j or P < 4):
                        continue
                    u, v = 0, 0
                    for s in (r, 2 * i, j):
                        dx, dy = tap(P, s)
                        v += dv(P, (par + u) & 1, dx, dy)
                        u += dy
                    hu, hv = max(hu, abs(u)), max(hv, abs(v))
    return hu, hv


def span(P):
    return abs(shear(P, tile_shape(P)[1] - 1))


def tile_grid(P, ah, astride):
    TW, TH = tile_shape(P)
    return (astride + span(P) + TW - 1) // TW, (ah + TH - 1) // TH      # tiles_x, tiles_y


def border(P, tx, ty, ah, astride):
    """The kernel's block-uniform `border`: does any staged position of tile (tx, ty) leave the image?  (arrays welcome)"""
    (TW, TH), (HU, HV) = tile_shape(P), HALO[P]
    bx0, by0 = tx * TW - (span(P) if K[P] > 0 else 0), ty * TH
    lo, hi = shear(P, -HU), shear(P, TH + HU)
    return ((by0 - HU < 0) | (by0 + TH + HU > ah) | (bx0 + min(0, lo) + min(0, hi) - HV - 1 < 0) |
            (bx0 + max(0, lo) + max(0, hi) + TW + HV + 1 > astride))


def tile_kinds(P, ah, astride):
    """(border tiles, interior tiles) of a padded frame."""
    nx, ny = tile_grid(P, ah, astride)
    ty, tx = np.mgrid[0:ny, 0:nx]
    b = border(P, tx, ty, ah, astride)
    return int(b.sum()), int((~b).sum())


def interior_mask(P, ah, astride):
    """(ah, astride) bool: the pixel is written by a tile that takes the interior form."""
    TW, TH = tile_shape(P)
    y, x = np.mgrid[0:ah, 0:astride]
    ty = y // TH
    sh = ((y - ty * TH) * K[P]) // 2
    tx = (x - sh + (span(P) if K[P] > 0 else 0)) // TW
    return ~border(P, tx, ty, ah, astride)


def interior_margin(P):
    """(rows, columns) from the frame's edges beyond which every pixel lies in an interior tile: a tile row plus its row halo;
    a tile column plus its column halo, the predicate's one spare column, the shear over the staged rows and the band's
    shift SPAN."""
    (TW, TH), (HU, HV) = tile_shape(P), HALO[P]
    return TH + HU, TW + HV + 1 + abs(shear(P, TH + HU)) + abs(shear(P, -HU)) + span(P)


# ---------------------------------------------------------------------------------------------- frames and parameters
def padded(size):
    d = O.calc_dim(*size)
    return d.ah, d.astride


FRAMES = [(1, 1), (33, 17), (8, 300), (300, 8), (200, 120)]
SHIFT_FRAME = (640, 360)
PADDED = {(1, 1): (32, 32), (33, 17): (48, 64), (200, 120): (144, 224), (640, 360): (384, 672)}      # (ah, astride), from the issue's table


def check_frame(size, P):
    """The frame still reaches, in direction P, the tile layouts it is in the list for."""
    ah, astride = padded(size)
    assert size not in PADDED or PADDED[size] == (ah, astride), (size, ah, astride)
    nx, ny = tile_grid(P, ah, astride)
    nb, ni = tile_kinds(P, ah, astride)
    if size == (1, 1):
        assert ni == 0 and (nx == 1 if P == 0 else ny == 1), (P, nx, ny, ni)
    elif size == (33, 17):
        assert ni == 0 and (ny == 2 if P else ny > 2), (P, nx, ny, ni)
    elif size == (8, 300):
        assert ny >= 10 and (nx == 1 if P == 0 else True), (P, nx, ny)
    elif size == (300, 8):
        assert nx >= 5 and (ny == 1 if P else True), (P, nx, ny)
    elif size == (200, 120):
        assert 72 <= nb <= 144 and 0 <= ni <= 72, (P, nb, ni)
        if P == 1:          # orders 0 and 2 launch whole groups of 8 / 64 workgroups: slots past the last tile
            assert nx * ny == 140 and nx * ny % 8 and nx * ny % 64
        if P in (0, 1, 5, 7):
            assert nb and ni, (P, nb, ni)
    return nx, ny, nb, ni


def default_sstd(size):
    return 6.0 * size[0] / 1920.0


PSETS = {
    'default': lambda size: (default_sstd(size), 0.05, 1.5, 0.8, 4.0),
    'sstd24': lambda size: (24.0, 0.05, 1.5, 0.8, 4.0),                # all 31 taps carry weight, the +-16 prefetch matters
    'dpow0': lambda size: (12.0, 0.1, 0.7, 0.0, 4.0),                  # w^0 = 1, also at w = 0
    'neg_gspeed': lambda size: (24.0, 0.05, 1.5, 0.8, -3.0),
}
KINDS = ('dense', 'sparse')


def scalars(pset, size):
    s = tuple(float(np.float32(v)) for v in PSETS[pset](size))
    if pset != 'default':
        assert math.exp(-225.0 / (M.RM_SQRT2 * s[0])) > 1e-9, 'tap 15 must carry weight'
    return s


@functools.lru_cache(maxsize=None)
def accumulator(kind, size, yuv=False):
    """The raw float32 accumulator (ah, astride, 4) of an input kind; read-only.  dense: synth_accum scaled to densities <= 64,
    through yuv_to_rgb (yuv = True: before it, for in_mode 2); sparse: sparse_accum with its 900-hit pixel set to 64 (yuv = True:
    the same values read as YUV, whose saturated colours clamp)."""
    d = O.calc_dim(*size)
    if kind == 'dense':
        acc = synth_accum(d, seed=11)
        acc = (acc * np.float32(64.0 / acc[:, 3].max())).astype(np.float32)
        if not yuv:
            acc = O.yuv_to_rgb(d, acc)
    else:
        acc = sparse_accum(d, seed=13).copy()
        assert (acc[:, 3] == 900.0).sum() == 1
        acc[acc[:, 3] == 900.0] *= np.float32(64.0 / 900.0)
    acc = np.ascontiguousarray(acc.reshape(d.ah, d.astride, 4))
    assert abs(acc[..., 3].max() - 64.0) < 1e-4 and (acc[..., 3] == 0).any() and (acc[..., 3] > 0).any()
    acc.setflags(write=False)
    return acc


def t_pow(raw, sc):
    """T_pow of the issue: the density factor's sensitivity to 2 ulp in each of log2 and exp2 of w^dpow,
    2 ln2 |0.5 / dstd| max_w w^dpow (ln2 dpow |log2 w| + 1) 2^-22, over the input's live densities."""
    w = np.asarray(raw, np.float64)[..., 3]
    w = w[w > 0]
    _, _, dstd, dpow, _ = sc
    return float(2 * math.log(2) * abs(0.5 / dstd) * (w ** dpow * (math.log(2) * dpow * np.abs(np.log2(w)) + 1)).max() * 2.0 ** -22)


FLOOR = 4 * 2.0 ** -24                             # tests/test_gpu_interp.py's floor
CAP = 1e-4                                         # a class that the oracle alone cannot keep under this is ill-conditioned


def _dim(H, W):
    return O.ref_dim(0, 0, 0, H, W)                # the oracle's filters read only the padded size (ah, astride)


def device_forms(P, raw32, in_mode=1):
    """What the device reads for direction P and what the model and the oracle read for the same picture: (device input float32
    (ah, astride, 4), model input float64 raw).  Direction 0 reads the raw accumulator (in_mode 2: in YUV, the model then
    reads the oracle's yuv_to_rgb of it); the others read its float32 normalised form, which the model un-normalises exactly."""
    if P == 0:
        if in_mode == 2:
            H, W = raw32.shape[:2]
            return raw32, np.asarray(O.yuv_to_rgb(_dim(H, W), np.ascontiguousarray(raw32.reshape(-1, 4))).reshape(H, W, 4), np.float64)
        return raw32, np.asarray(raw32, np.float64)
    n32 = M.to_normalised(raw32).astype(np.float32)
    return n32, M.to_raw(n32)


def out_form(P, raw_out, S):
    """A raw float64 result in the form direction P stores: raw for direction 7, normalised for the others."""
    return np.asarray(raw_out, np.float64) if P == 7 else M.normalised_out(raw_out, S)


def oracle_pass(raw64, P, sc):
    H, W = raw64.shape[:2]
    src = np.ascontiguousarray(raw64.reshape(-1, 4), np.float32)
    return O.bilateral_pass(_dim(H, W), src, P, *sc)[0].reshape(H, W, 4)


_A = {}


def case_a(P, size, kind, pset, in_mode=1):
    """Section A / E: (device input, model result in the direction's output form, e_oracle, T_pow), computed once per session."""
    key = (P, size, kind, pset, in_mode)
    if key not in _A:
        sc = scalars(pset, size)
        dev_in, raw64 = device_forms(P, accumulator(kind, size, yuv=in_mode == 2), in_mode)
        out, S = M.bilateral_pass(raw64, P, sc)
        want = out_form(P, out, S)
        e = M.ratio(out_form(P, oracle_pass(raw64, P, sc), S), want)[0]
        want.setflags(write=False)
        _A[key] = (dev_in, want, e, t_pow(raw64, sc))
    return _A[key]


@functools.lru_cache(maxsize=None)
def bound(fam, kind, pset):
    """B of a class (direction family x input kind x parameter set) over every direction of the family and every frame:
    (B, e_oracle, T_pow) with B = max(4 e_oracle + T_pow, FLOOR).  e_oracle is the float32 oracle's own worst ratio against the
    model on the same inputs; the margin of 4 is test_gpu_interp.py's (hardware exp2 / rcp / log2 are 1-2 ulp where libm is 0.5)."""
    if kind == 'lone':
        rows = [lone_case(P, size, sstd)[1:] for P in FAMILIES[fam] for size in FRAMES for sstd in LONE_SSTD]
    else:
        rows = [case_a(P, size, kind, pset)[2:] for P in FAMILIES[fam] for size in FRAMES]
    e, t = max(r[0] for r in rows), max(r[1] for r in rows)
    return max(4 * e + t, FLOOR), e, t


# ---------------------------------------------------------------------------------------------- B: lone bins
LONE = np.float32([0.3, 0.5, 0.2, 1.0])
LONE_SSTD = (24.0, 6.0)                            # (at the default 0.625 underflow cuts the support to 17 taps)
LONE_APART = 64


def lone_scalars(sstd):
    return (sstd, 0.05, 1.5, 0.8, 4.0)


def lone_points(size):
    """[[(y, x)]]: per accumulator the positions of its lone bins, pairwise at least LONE_APART apart (in x or in y).
    At 200 x 120, 22 accumulators of bins on a 65 x 80 grid whose origin moves so that the bins sweep every column residue
    mod 64 and every row residue mod 32 (so: every column and row of a 64 x 4 and of an 8 x 32 tile, both row parities); at every
    size, bins on the four corners and the four edge midpoints."""
    H, W = padded(size)
    frames = []
    if size == (200, 120):
        for f in range(22):
            jx, jy = 3 * f, f % 16
            frames.append([(24 + jy + 80 * j, 15 + jx + 65 * i) for j in range(2) for i in range(3)])      # all 15 or more from an edge
    edge = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    groups = []
    for p in edge:
        for g in groups:
            if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= LONE_APART for q in g):
                g.append(p)
                break
        else:
            groups.append([p])
    return frames + groups


def support(P, H, W, pts):
    """(H, W) bool: the pixels one of whose 31 clamped taps lands on a bin — away from the edges the 31 pixels q - t(r)."""
    live = np.zeros((H, W), bool)
    for y, x in pts:
        live[y, x] = True
    ys, xs = np.arange(H), np.arange(W)
    m = np.zeros((H, W), bool)
    for dx, dy in M.tap_offsets(P):
        m |= live[np.ix_(np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1))]
    return m


_L = {}


def lone_case(P, size, sstd):
    """([(device input, support mask, model values on the support in P's output form, bin positions)] per accumulator, e_oracle,
    T_pow); the oracle is also held to the exact support here."""
    key = (P, size, sstd)
    if key not in _L:
        H, W = padded(size)
        sc = lone_scalars(sstd)
        frames, es = [], []
        for pts in lone_points(size):
            raw = np.zeros((H, W, 4), np.float32)
            for y, x in pts:
                raw[y, x] = LONE
            dev_in, raw64 = device_forms(P, raw)
            sup = support(P, H, W, pts)
            ys, xs = np.nonzero(sup)
            out, S = M.bilateral_at(raw64, P, sc, ys, xs)
            want = out_form(P, out, S)
            orc = oracle_pass(raw64, P, sc)
            assert not orc[~sup].any(), 'the oracle writes outside the support'
            es.append(M.ratio(out_form(P, orc[ys, xs], S), want)[0])
            frames.append((dev_in, sup, want, pts))
        _L[key] = (frames, max(es), t_pow(LONE[None, None], sc))
    return _L[key]


def check_lone(P, size, sstd):
    """Every bin away from the edges has exactly the 31 pixels q - t(r) as its support, each with a model density far from
    flush-to-zero; every accumulator holds fewer live pixels than a wave has lanes, so every wave that computes has a dead
    centre and takes de_tap_loop_slow — in border tiles and, where the frame has them, interior tiles."""
    H, W = padded(size)
    frames = lone_case(P, size, sstd)[0]
    n_inner, smallest = 0, 1.0
    for dev_in, sup, want, pts in frames:
        assert (dev_in[..., 3] > 0).sum() == len(pts) < 64
        for y, x in pts:
            if 15 <= y < H - 15 and 15 <= x < W - 15:
                mine = {(y - dy, x - dx) for dx, dy in M.tap_offsets(P)}
                assert len(mine) == 31 and all(sup[p] for p in mine)
                n_inner += 1
        ys, xs = np.nonzero(sup)
        inner = (ys >= 30) & (ys < H - 30) & (xs >= 30) & (xs < W - 30)
        if inner.any():
            smallest = min(smallest, want[inner, 3].min())
            assert smallest > (1e-5 if sstd == 24.0 else 1e-13), smallest
    if size == (200, 120):
        cols = {x % 64 for f in frames[:22] for y, x in f[3]}
        rows = {y % 32 for f in frames[:22] for y, x in f[3]}
        assert cols == set(range(64)) and rows == set(range(32)) and n_inner >= 22 * 6
        im = interior_mask(P, H, W)
        hit = np.zeros((H, W), bool)
        for f in frames:
            hit |= f[1]
        nb, ni = tile_kinds(P, H, W)
        assert (hit & ~im).any() and ((hit & im).any() or ni == 0), 'a support in each kind of tile'
    return n_inner, smallest


# ---------------------------------------------------------------------------------------------- C: shifts
SHIFT_RECT = (96, 288, 192, 480)                   # rows, columns of the padded 672 x 384 frame compared
PICTURE = (160, 224)                               # rows, columns of the picture, placed at the rectangle's corner + the shift


def shifts(P):
    """(sx, sy): every column residue of the direction's tile at sy = 0, every row residue at sx = 0, and a diagonal walk
    through min(TW * TH, 64) distinct residue pairs."""
    TW, TH = tile_shape(P)
    walk = [(k % TW, (k + k // TW) % TH) for k in range(min(TW * TH, 64))]
    assert len(set(walk)) == len(walk)
    out = [(sx, 0) for sx in range(1, TW)] + [(0, sy) for sy in range(1, TH)] + [s for s in walk if s[0] and s[1]]
    return out


@functools.lru_cache(maxsize=None)
def shift_picture(kind):
    """Full-range densities (to 2000): a window of synth_accum / sparse_accum at 640 x 360 that holds live and empty pixels."""
    d = O.calc_dim(*SHIFT_FRAME)
    acc = (O.yuv_to_rgb(d, synth_accum(d, seed=11)) if kind == 'dense' else sparse_accum(d, seed=13)).reshape(d.ah, d.astride, 4)
    y0, x0 = (60, 200) if kind == 'dense' else (110, 20)
    pic = np.ascontiguousarray(acc[y0:y0 + PICTURE[0], x0:x0 + PICTURE[1]])
    w = pic[..., 3]
    assert (w == 0).mean() > 0.05 and (w > 0).mean() > (0.05 if kind == 'dense' else 0.005), (kind, (w == 0).mean())
    assert w.max() >= (200.0 if kind == 'dense' else 900.0), (kind, w.max())
    pic.setflags(write=False)
    return pic


def shift_input(P, kind, sx, sy):
    """The picture at (sx, sy) from the compared rectangle's corner in an empty 672 x 384 frame, in the form direction P reads."""
    H, W = padded(SHIFT_FRAME)
    buf = np.zeros((H, W, 4), np.float32)           # (an empty pixel is (0, 0, 0, 0) in both forms)
    y0, x0 = SHIFT_RECT[0] + sy, SHIFT_RECT[2] + sx
    buf[y0:y0 + PICTURE[0], x0:x0 + PICTURE[1]] = _shift_picture_form(kind, P == 0)
    return buf


@functools.lru_cache(maxsize=None)
def _shift_picture_form(kind, raw):
    return shift_picture(kind) if raw else M.to_normalised(shift_picture(kind)).astype(np.float32)


def check_shift(P):
    """The compared rectangle lies in interior tiles for every shift of the list, the picture and the reach of its pixels'
    results stay inside it, and the margin that makes it so follows from the halo and the shear."""
    H, W = padded(SHIFT_FRAME)
    my, mx = interior_margin(P)
    TW, TH = tile_shape(P)
    r0, r1, c0, c1 = SHIFT_RECT
    assert my <= r0 and mx <= c0 and r1 <= H - my and c1 <= W - mx, (P, my, mx)
    assert interior_mask(P, H, W)[my:H - my, mx:W - mx].all(), P
    assert not interior_mask(P, H, W)[:, 0].any() and not interior_mask(P, H, W)[:, W - 1].any()
    assert r0 + PICTURE[0] + TH - 1 <= r1 and c0 + PICTURE[1] + TW - 1 <= c1
    return my, mx
