"""
The test flames: genome and profile builders and their constants, shared by the CPU tests, the GPU tests and tools/.
Nothing here opens the device.
"""
import copy
import json
import os

import numpy as np

from cuburn_amd import configs
from cuburn_amd.genome import variations as V
import chaos_model as X

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def small(cfg, w, h, **kw):
    gnm, prof = cfg(**kw)
    prof = dict(prof, width=w, height=h)
    return gnm, prof


def linear_flame():
    """3 linear xforms + post affine + final xform: no transcendentals anywhere => bit-exact."""
    gnm, prof = configs.cfg2()
    for k in gnm['xforms']:
        gnm['xforms'][k]['variations'] = {'linear': {'weight': 0.8}, 'bent': {'weight': 0.2}}
    gnm['xforms']['1']['post_affine'] = configs._affine(10.0, 0.9, 0.05, -0.1)
    gnm['final_xform'] = {'color': 0.3, 'color_speed': 0.25, 'pre_affine': configs._affine(-8.0, 0.97, 0.02, 0.01),
                          'variations': {'linear': {'weight': 1.0}}}
    return gnm, dict(prof, width=1280, height=720)


def animated_linear_flame():
    """The transcendental-free flame in motion: camera pan, one rotating xform, two palettes, a
    frame window that spans the whole animation: every slot sees a different parameter block
    and the 64 palette rows differ."""
    gnm, prof = linear_flame()
    gnm['camera']['center'] = {'x': [-0.15, 0.3, 0.15, 0.3], 'y': 0.0}
    gnm['camera']['scale'] = 1.0          # zoomed in: every cell stays below the packed-add limit of the binned drain
    gnm['xforms']['0']['pre_affine']['angle'] = [70.0, 30.0, 100.0, 30.0]
    gnm['palette'] = [configs._pal(0.0, configs.fire_palette()), configs._pal(1.0, configs.ice_palette())]
    gnm['time'] = {'duration': 1, 'frame_width': 1.0}
    return gnm, dict(prof, frame_width=1.0, fps=1, duration=1)


def hot_flame():
    """The transcendental-free flame plus a strongly contracting xform: a ~100-pixel region that
    takes 3 % of all samples."""
    gnm, prof = linear_flame()
    gnm['xforms']['3'] = {'weight': 0.031, 'color': 0.8, 'color_speed': 0.5,
                          'pre_affine': configs._affine(15.0, 0.05, 0.3, -0.2),
                          'variations': {'linear': {'weight': 1.0}}}
    return gnm, dict(prof, width=512, height=512)


def point_flame(share):
    """The transcendental-free flame plus an xform that maps everything onto ONE point: that pixel
    takes about `share` of all samples (share 1: the point xform alone)."""
    gnm, prof = linear_flame()
    point = {'weight': 1.0, 'color': 0.8, 'color_speed': 0.5, 'pre_affine': configs._affine(0.0, 0.0, 0.21, -0.13),
             'variations': {'linear': {'weight': 1.0}}}
    if share >= 1.0:
        gnm['xforms'] = {'0': point}
    else:
        total = sum(x['weight'] for x in gnm['xforms'].values())
        gnm['xforms']['3'] = dict(point, weight=total * share / (1.0 - share))
    return gnm, dict(prof, width=512, height=512)


def animated_cfg5():
    """cfg5's twelve heavy xforms (more than the per-genome kernel keeps resident: records fetched per round, operand table in LDS)
    with a moving xform, a moving offset and a turning camera, so that every temporal sample has its own parameter block."""
    gnm, prof = configs.cfg5(samples=2 ** 26)
    gnm['time'] = {'duration': 1, 'frame_width': 1.0}
    gnm['camera'] = dict(gnm['camera'], rotation=[0.0, 15.0, 15.0, 15.0])
    gnm['xforms']['03']['pre_affine']['angle'] = [30.0, 50.0, 80.0, 50.0]
    gnm['xforms']['07']['pre_affine']['offset']['x'] = [-0.3, 0.5, 0.2, 0.5]
    return gnm, dict(prof, frame_width=1.0, fps=24, duration=2)


def nxf_flame(n, w=256, h=144):
    """n linear xforms on a ring, unequal weights (the density table has n-1 entries)."""
    gnm, prof = configs.cfg1()
    xfs = {}
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1)
        xfs[str(i)] = {'weight': 0.2 + (i % 5) * 0.3, 'color': i / max(n - 1, 1), 'color_speed': 0.5,
                       'pre_affine': configs._affine(7.0 * i, 0.45, 0.55 * float(np.cos(a)), 0.55 * float(np.sin(a))),
                       'variations': {'linear': {'weight': 1.0}}}
    gnm['xforms'] = xfs
    return gnm, dict(prof, width=w, height=h)


BOX_OFFSETS = ((-0.45, -0.3), (0.45, -0.3), (0.0, 0.42))
BOX_WEIGHTS = (0.5, 0.3, 0.2)
# Pixel rectangles (rows, columns; inclusive) of the padded accumulator (272 rows of 352, 344 columns in use) that hold the three disjoint images of the
# attractor's hull, found with the CPU oracle at 2^24 samples: the box of xform `2`, and the two lower boxes (which of them
# is xform `0` follows from the camera's sign conventions; the GPU test reads it off the keyless render's masses).
BOX_TOP = (80, 118, 148, 196)
BOX_LOW_LEFT = (138, 176, 112, 160)
BOX_LOW_RIGHT = (138, 176, 184, 232)


def three_boxes(opacity=None, samples=2 ** 26):
    """Three linear xforms whose images are disjoint: a plotted sample lies in box k exactly when xform k produced it, so
    without opacity box k holds the fraction w_k of what is plotted, and with opacities q_k w_k / sum_j q_j w_j.
    ``opacity``: None (no key anywhere) or one value per xform (None: no key on that xform)."""
    xforms = {}
    for k, ((ox, oy), w) in enumerate(zip(BOX_OFFSETS, BOX_WEIGHTS)):
        xforms[str(k)] = {'weight': w, 'color': 0.5 * k, 'color_speed': 0.5,
                          'pre_affine': configs._affine(0, 0.4, ox, oy), 'variations': {'linear': {'weight': 1.0}}}
        if opacity is not None and opacity[k] is not None:
            xforms[str(k)]['opacity'] = opacity[k]
    gnm = {'type': 'animation', 'name': 'three-boxes',
           'camera': {'center': {'x': 0.0, 'y': 0.0}, 'rotation': 0.0, 'scale': 0.25},
           'time': {'duration': 1, 'frame_width': 0.0},
           'palette': [configs._pal(0.0, configs.grey_ramp())], 'xforms': xforms}
    prof = {'width': 320, 'height': 240, 'spp': samples / (320.0 * 240.0), 'fps': 1, 'duration': 1, 'frame_width': 0,
            'output': {'type': 'raw'}, 'filter_order': ['bilateral', 'logscale', 'colorclip']}
    return gnm, prof


def plot_probability(p):
    """The contract's q(p) in float64."""
    p = min(max(float(p), 0.0), 1.0)
    if p <= 0.0:
        return 0.0
    if p >= float(np.float32(1) - np.float32(1e-6)):          # (the snap's threshold is the float32 number, 0.99999899)
        return 1.0
    q = 10.0 ** np.log2(p)
    return 0.0 if q < 2.0 ** -32 else q


def with_opacity(gnm, keys, value=0.5):
    gnm = copy.deepcopy(gnm)
    for k in keys:
        gnm['xforms'][k]['opacity'] = value
    return gnm


FRACTIONAL = [[1.0, 0.5, 2.0], [0.25, 1.0, 1.0], [1.0, 3.0, 0.5]]
FORBIDDEN = [[0.5, 1.0, 0.0], [1.0, 1.0, 2.0], [1.0, 0.0, 1.0]]          # 0 -> 2 and 2 -> 1 never happen; lambda = 0.31
ZERO_DIAGONAL = [[0.0, 1.0, 1.0], [1.0, 0.0, 0.5], [2.0, 1.0, 0.0]]      # no xform follows itself (lambda = 0.81: exact tests only)
CYCLE = [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]              # 0 -> 1 -> 2 -> 0


def many_xforms(n, chaos):
    gnm, prof = X.nine_boxes()
    xf = gnm['xforms']['0']
    gnm['xforms'] = dict(('%02d' % i, copy.deepcopy(xf)) for i in range(n))
    if chaos:
        gnm['xforms']['00']['chaos'] = {'01': 0.5}
    return gnm, prof


def rich_xml():
    src = json.load(open(os.path.join(GOLD, 'genome_front.json')))['xml']['rich']
    assert src.count(' chaos="1 0.5 2"') == 1
    return src


SPREAD_SIZE = (256, 256)


def spread_flame(table):
    """cfg2 (linear, spherical, swirl) with a chaos table at 256 x 256, zoomed in: many lit cells below the drain threshold for
    the atomic comparisons (the nine boxes' attractor is a dust of ~200 hot pixels), and samples out of frame."""
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=SPREAD_SIZE[0], height=SPREAD_SIZE[1], spp=2 ** 22 / float(SPREAD_SIZE[0] * SPREAD_SIZE[1]))
    gnm['camera']['scale'] = 0.5
    for p, k in enumerate(sorted(gnm['xforms'])):
        gnm['xforms'][k]['chaos'] = dict((str(n), v) for n, v in enumerate(table[p]))
    return gnm, prof


# variations that are safe to draw at random weights (bounded output for bounded input or
# at least not systematically divergent); the full set is covered one by one in
# test_gpu_variations.py
POOL = ['linear', 'sinusoidal', 'spherical', 'swirl', 'horseshoe', 'polar', 'handkerchief', 'heart', 'disc',
        'spiral', 'hyperbolic', 'diamond', 'ex', 'julia', 'bent', 'waves', 'fisheye', 'popcorn', 'power',
        'cosine', 'rings', 'fan', 'blob', 'pdj', 'fan2', 'rings2', 'eyefish', 'bubble', 'cylinder',
        'perspective', 'julian', 'juliascope', 'ngon', 'curl', 'rectangles', 'tangent', 'cross', 'cell',
        'bipolar', 'wedge', 'scry', 'split', 'stripes', 'waves2', 'mobius', 'flux']


def random_spline(rs, lo, hi, animated):
    a = float(rs.uniform(lo, hi))
    if not animated or rs.rand() < 0.5:
        return a
    b = float(rs.uniform(lo, hi))
    span = hi - lo
    knots = [a, float(rs.uniform(-0.3, 0.3) * span), b, float(rs.uniform(-0.3, 0.3) * span)]
    if rs.rand() < 0.4:                      # an interior knot
        knots += [float(rs.uniform(0.2, 0.8)), float(rs.uniform(lo, hi))]
    return knots


def random_genome(seed):
    rs = np.random.RandomState(seed)
    animated = seed % 2 == 1
    nxf = int(rs.randint(1, 13))
    xforms = {}
    for i in range(nxf):
        names = list(rs.choice([n for n in POOL if n in V.var_ids], size=int(rs.randint(1, 4)), replace=False))
        if rs.rand() < 0.5 and 'linear' not in names:
            names.append('linear')
        var = {}
        for n in names:
            var[n] = {'weight': random_spline(rs, 0.2, 0.9, animated)}
            for p, (dflt, interp) in V.var_params[n].items():
                if p != 'weight' and rs.rand() < 0.7:
                    base = dflt if dflt else 0.5
                    var[n][p] = random_spline(rs, 0.5 * base, 1.5 * base, animated) if interp == 'mag' else \
                        random_spline(rs, -abs(base), abs(base), animated)
        xf = {'weight': random_spline(rs, 0.1, 1.0, animated), 'color': random_spline(rs, 0.0, 1.0, animated),
              'color_speed': random_spline(rs, 0.1, 0.9, animated),
              'pre_affine': configs._affine(float(rs.uniform(-180, 180)), float(rs.uniform(0.3, 0.8)),
                                            float(rs.uniform(-0.6, 0.6)), float(rs.uniform(-0.5, 0.5))),
              'variations': var}
        if animated and rs.rand() < 0.5:
            xf['pre_affine']['angle'] = [xf['pre_affine']['angle'], float(rs.uniform(-90, 90)),
                                         xf['pre_affine']['angle'] + float(rs.uniform(-60, 60)), float(rs.uniform(-90, 90))]
        if rs.rand() < 0.4:
            xf['post_affine'] = configs._affine(float(rs.uniform(-30, 30)), float(rs.uniform(0.8, 1.1)),
                                                float(rs.uniform(-0.1, 0.1)), float(rs.uniform(-0.1, 0.1)))
        xforms[str(i)] = xf
    gnm = {'type': 'animation', 'name': 'random-%d' % seed,
           'camera': {'center': {'x': random_spline(rs, -0.2, 0.2, animated), 'y': random_spline(rs, -0.2, 0.2, animated)},
                      'rotation': random_spline(rs, -40, 40, animated), 'scale': random_spline(rs, 0.15, 0.35, animated)},
           'time': {'duration': 2, 'frame_width': 1.0 if animated else 0.0},
           'palette': [[0.0] + configs.palette_encode(configs.grey_ramp())],
           'xforms': xforms}
    if animated:
        ramp = configs.grey_ramp()[::-1].copy()
        gnm['palette'].append([1.0] + configs.palette_encode(ramp))
    if rs.rand() < 0.4:
        gnm['final_xform'] = {'color': 0.2, 'color_speed': float(rs.uniform(0, 0.5)),
                              'pre_affine': configs._affine(float(rs.uniform(-10, 10)), float(rs.uniform(0.9, 1.1)), 0.0, 0.0),
                              'variations': {'linear': {'weight': 1.0}}}
    prof = {'width': 384, 'height': 216, 'spp': 2 ** 24 / (384.0 * 216.0), 'fps': 24, 'duration': 2,
            'frame_width': 1.0 if animated else 0.0, 'output': {'type': 'raw'},
            'filter_order': ['bilateral', 'logscale', 'colorclip']}
    return gnm, prof
