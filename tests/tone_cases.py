"""
Inputs and metrics shared by tests/test_cpu_tone.py and tests/test_gpu_tone.py: the atlas of pixels, the grids of scalars, and the
deviation of an evaluation from the float64 model of tests/tone_model.py per branch class.
"""
import numpy as np

from common import O
from cuburn_amd import configs, filters, profile, render
import tone_model as TM

AW, AH = 40, 8                                            # calc_dim(40, 8): astride 64, ah 32 -> the atlas fills the buffer exactly
RATIOS = [0.0, 0.05, 0.5, 0.95, 1.0, 1.3, 3.0, 8.0]       # max colour over density
SHAPES = [(1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.5), (0.2, 0.6, 1.0)]

VIBS = [1.0, 0.9, 0.5, 0.0]
HIGHPOWS = [-2.0, -1.0, -0.5, 0.0, 1.5, 3.0]
GAMLINS = [(0.25, 0.01), (1.0 / 3.0, 0.02), (0.9, 0.0), (0.1, 0.3), (1.0, 0.05)]
LOG_K1, LOG_K2 = 4.1875, 0.02                             # the logscale in front of the clips

RELATIVE = ('logscale', 'smearclip', 'haloclip', 'plainclip')
# Added to |model| in the relative metric.  The tails of smearclip's blurs underflow float32 (the outer coefficient of the 0.3-wide
# gaussian is 2e-22, and four blurs multiply): flush-to-zero is the contract there, the float64 model keeps 1e-60.  Everything a
# filter computes without underflow is above 1e-13 on these inputs, so the term changes nothing else.
UNDERFLOW = 1e-25


# ------------------------------------------------------------------ inputs shared with tests/test_gpu_tone.py
def densities(lo=-4.0, hi=1.5):
    return np.concatenate([[0.0], np.logspace(lo, hi, 63)]).astype(np.float32)


def atlas(dens=None):
    """(2048, 4) float32: pixel 32 r + 4 i + j has density dens[r] and colour RATIOS[i] * dens[r] * SHAPES[j]; the empty row
    (density 0) carries the colours of density 1, which every filter must drop."""
    dens = densities() if dens is None else np.asarray(dens, np.float32)
    assert dens.shape == (64,)
    col = (np.array(RATIOS, np.float32)[:, None, None] * np.array(SHAPES, np.float32)[None]).reshape(32, 3)
    buf = np.zeros((64, 32, 4), np.float32)
    buf[..., 3] = dens[:, None]
    buf[..., :3] = np.where(dens > 0, dens, np.float32(1))[:, None, None] * col[None]
    buf = buf.reshape(-1, 4)
    assert not ((buf != 0) & (np.abs(buf) < np.finfo(np.float32).tiny)).any()
    return buf


def wide_atlas():
    """The atlas over densities 1e-6 .. 3e8: what the DE leaves at the rim of a flame, and a point attractor's bin."""
    return atlas(np.concatenate([[0.0], np.logspace(-6.0, np.log10(3e8), 63)]))


def yuv_atlas():
    """The atlas read as (Y, U, V, w) with U - w / 2 and V - w / 2 of either sign (the four sign pairs by density row)."""
    buf = atlas()
    r = np.arange(2048) // 32
    su = np.where(r % 2 == 0, 1, -1).astype(np.float32)
    sv = np.where(r // 2 % 2 == 0, 1, -1).astype(np.float32)
    out = buf.copy()
    out[:, 1] = np.float32(0.5) * buf[:, 3] + su * buf[:, 1]
    out[:, 2] = np.float32(0.5) * buf[:, 3] + sv * buf[:, 2]
    return out


def colorclip_grid():
    """The 120 scalar sets [vib, highpow, gam, lin, lingam], as float32."""
    return [[np.float32(v), np.float32(hp), np.float32(g), np.float32(l), TM.lingam_of(g, l)]
            for v in VIBS for hp in HIGHPOWS for g, l in GAMLINS]


def clip_cases():
    """(filter, float32 scalars) of the plain clips: the five (gam, lin) pairs, three smear widths, two brightnesses."""
    out = []
    for g, l in GAMLINS:
        gm1, lin, lingam = np.float32(np.float32(g) - 1), np.float32(l), TM.lingam_of(g, l)
        out += [('smearclip', [np.float32(wd), gm1, lin, lingam]) for wd in (0.3, 0.7, 2.0)]
        out += [('haloclip', [gm1])]
        out += [('plainclip', [gm1, lin, lingam, np.float32(b)]) for b in (0.5, 4.0)]
    return out


def logscaled(buf):
    """The model's logscale of a buffer, as the float32 input of the clips."""
    return TM.logscale(buf, LOG_K1, LOG_K2).astype(np.float32)


def config_k2s():
    """k2 as Logscale.scalars derives it for cfg1 .. cfg5, plus 1e-6."""
    out = []
    for name in ('cfg1', 'cfg2', 'cfg3', 'cfg4', 'cfg5'):
        gnm, prof = configs.CONFIGS[name]()
        gprof = profile.wrap(prof, gnm)
        dim = render.Framebuffers.calc_dim(gprof.width, gprof.height)
        out.append(filters.Logscale().scalars(gprof, gprof.filters.logscale, dim, 0.5)[1])
    return out + [np.float32(1e-6)]


def model_clip(name, buf, ah, astride, vals):
    """(model output, classes) of one of the plain clips."""
    if name == 'smearclip':
        return TM.smearclip_chain(buf, ah, astride, *vals)
    if name == 'haloclip':
        return TM.haloclip_chain(buf, ah, astride, *vals)
    return TM.plainclip(buf, *vals), TM.clip_classes(buf[:, 3].astype(np.float64), vals[1])


def oracle_clip(name, d, buf, vals):
    return {'smearclip': O.smearclip_chain, 'haloclip': O.haloclip_chain, 'plainclip': O.plainclip}[name](d, buf, *vals)


def yuv_ulps(got, model, src):
    """|got - model| in float32 ulp of the pixel's largest input magnitude.  Y - 0.34414 u - 0.71414 v cancels, and the clamp cuts
    results off at 0: no float32 sum is accurate in ulp of such a RESULT, only in ulp of its largest term, which is where each of
    its roundings happens.  Where nothing cancels the two are the same."""
    scale = np.abs(src.astype(np.float64)).max(1)
    ulp = 2.0 ** (np.floor(np.log2(np.where(scale > 0, scale, 1.0))) - 23)
    return np.abs(got.astype(np.float64) - model) / ulp[:, None]


def deviation(name, got, model, cls, src=None):
    """Worst deviation of `got` from the model per branch class, {class name: value}, in the filter's metric (see ORACLE_DEV in tests/test_cpu_tone.py).
    Where the model is exactly 0 (empty pixels, black channels) or infinite, `got` must equal it: asserted here."""
    got64 = np.asarray(got).astype(np.float64)
    exact = (model == 0) | ~np.isfinite(model)                     # (a blur tail below float32's range is not 0: see UNDERFLOW)
    if name == 'yuv':
        exact[:] = False                                           # (a clamped 0 is the end of a sum like any other value)
    assert np.array_equal(got64[exact], model[exact]), '%s: %d values differ where the model is 0 / inf' % (
        name, (got64[exact] != model[exact]).sum())
    assert np.isfinite(got64[~exact]).all(), '%s: non-finite values where the model is finite' % name
    if name == 'yuv':
        err = yuv_ulps(got, model, src)
    else:
        with np.errstate(invalid='ignore'):
            err = np.abs(got64 - model)                            # (inf - inf where both are -inf: masked below)
        if name in RELATIVE:
            err = err / (np.abs(model) + UNDERFLOW)
    err = np.where(exact, 0.0, err).max(1)
    return {TM.CLASS_NAMES[c]: float(err[cls == c].max()) for c in np.unique(cls) if c != TM.EMPTY}


def scale_of(name, model, cls):
    """max |model| per class: what the floor of an absolute bar is taken from (1 for the relative metrics and yuv's ulp)."""
    if name in RELATIVE or name == 'yuv':
        return {TM.CLASS_NAMES[c]: 1.0 for c in np.unique(cls) if c != TM.EMPTY}
    m = np.where(np.isfinite(model), np.abs(model), 0.0).max(1)
    return {TM.CLASS_NAMES[c]: float(m[cls == c].max()) for c in np.unique(cls) if c != TM.EMPTY}


def merge(worst, name, dev):
    for k, v in dev.items():
        worst[(name, k)] = max(worst.get((name, k), 0.0), v)


def reachable(highpow):
    if highpow >= 0:
        return [TM.HIGHLIGHT, TM.PLAIN, TM.HIGHLIGHT_LIN, TM.PLAIN_LIN]
    if highpow > -1:
        return [TM.BLENDED, TM.PLAIN, TM.BLENDED_LIN, TM.PLAIN_LIN]
    return [TM.PLAIN, TM.PLAIN_LIN]


LIVE = np.ones(2048, np.int64) * TM.PLAIN
