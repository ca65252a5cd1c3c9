"""
numpy model of the tone-mapping filters in float64: the contract the HIP kernels (cuburn_amd/csrc/tone_device.h, filters.hip and
the tail of de.hip's last direction) and the float32 oracle (oracle/filters_ref.c) are both held to.  Written from the formulas of
the reference, at the lines the kernels cite:

  yuv_to_rgb        cuburn/code/filters.py:71-77 (+ the YUV matrix of cuburn/code/color.py:25-40)
  logencode         cuburn/code/filters.py:81-90
  logscale          cuburn/code/filters.py:41-53
  haloclip_chain    cuburn/code/filters.py:268-288, launch order cuburn/filters.py:113-130
  smearclip_chain   cuburn/code/filters.py:294-328, launch order cuburn/filters.py:142-163
  plainclip         cuburn/code/filters.py:332-350
  colorclip         cuburn/code/filters.py:354-412
  gauss_coefs       cuburn/filters.py:11-16

Images are the padded buffers, (ah * astride, 4) arrays (colour in [:, :3], density in [:, 3]).  Inputs are float32 data and are
exact in float64; every scalar enters as the float32 value the host passes (np.float32(x) widened), and everything after that is
float64.  Decisions (w < lin, maxa > 1, w > 0) are taken on the float64 values: tests/test_cpu_tone.py shows every filter to be
continuous across those seams, so a float32 evaluation that decides the other way one ulp from a seam lands within a few ulp.
"""
import numpy as np

# cuburn/code/filters.py:8-17: the four shear patterns the tone filters blur along (x step, y step per tap)
PATTERNS = [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (-1.0, 1.0)]

# branch classes of colorclip (and, 0 .. 2 of them, of the plain clips: EMPTY, PLAIN, PLAIN_LIN)
EMPTY, HIGHLIGHT, BLENDED, PLAIN, HIGHLIGHT_LIN, BLENDED_LIN, PLAIN_LIN = range(7)
CLASS_NAMES = ['empty', 'highlight', 'blended', 'plain', 'highlight<lin', 'blended<lin', 'plain<lin']


def _s(x):
    """A host scalar as the kernel receives it: rounded to float32, then exact in float64."""
    return float(np.float32(x))


def _buf(buf):
    b = np.asarray(buf)                 # float32 data, or the float64 output of the stage in front
    assert b.dtype in (np.float32, np.float64) and b.ndim == 2 and b.shape[1] == 4
    return b.astype(np.float64)


def lingam_of(gam, lin):
    """cuburn/filters.py:132-136: lin^(gam - 1) from the float32 gam and lin, 0 at lin == 0, as a float32."""
    gam, lin = np.float32(gam), np.float32(lin)
    return np.float32(float(lin) ** (float(gam) - 1.0) if lin > 0 else 0.0)


def gauss_coefs(stdev):
    """The 7 blur coefficients exp(-x^2 / (2 stdev^2)), x = -3 .. 3, normalised to sum 1.  They are host scalars like the others:
    the host derives them in float32 from the float32 width and the kernels receive those values, so they are formed in float32
    here too and widened.  (The outer coefficient of a 0.3-wide gaussian is e^-50: one float32 rounding of 2 stdev^2 moves it by
    5e-6 of itself, and a float64 restatement would measure that rounding, not the kernels.)"""
    s = np.float32(stdev)
    x = np.arange(-3, 4).astype(np.float32)
    c = np.exp(x * x / (np.float32(-2.0) * s * s)).astype(np.float32)
    return (c / c.sum(dtype=np.float32)).astype(np.float64)


def yuv_to_rgb(buf):
    p = _buf(buf)
    y, w = p[:, 0], p[:, 3]
    u, v = p[:, 1] - _s(0.5) * w, p[:, 2] - _s(0.5) * w
    out = np.empty_like(p)
    out[:, 0] = np.maximum(0.0, y + _s(1.402) * v)
    out[:, 1] = np.maximum(0.0, y - _s(0.34414) * u - _s(0.71414) * v)
    out[:, 2] = np.maximum(0.0, y + _s(1.772) * u)
    out[:, 3] = w
    return out


def logscale(buf, k1, k2):
    """p * max(0, k1 log(1 + w k2) / w), 0 at w == 0.

    The sum s = 1 + w k2 is part of the operation's float32 definition: it is formed in float32 (the product rounded, then the
    sum), and only the logarithm of that float32 s and what follows are float64.  With a float64 sum the model would keep w k2
    below 2^-24, which every float32 evaluation (the reference's included) rounds away: the two would differ by 100 % there, and
    by the rounding of s relative to w k2 everywhere near 1.  That is the operation, not an error of whoever evaluates it."""
    p = _buf(buf)
    w32 = np.asarray(buf)[:, 3]
    s = (np.float32(1.0) + w32 * np.float32(k2)).astype(np.float32).astype(np.float64)
    w = p[:, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        ls = np.where(w != 0, _s(k1) * np.log(s) / w, 0.0)
    return p * np.maximum(0.0, ls)[:, None]


def _clip_ls(w, gam_m_1, lin, lingam):
    """w^(gam - 1), blended with lingam below lin (cuburn/code/filters.py:321-325, :343-347); w > 0."""
    ls = w ** gam_m_1
    if lin > 0:
        frac = w / lin
        ls = np.where(w < lin, (1.0 - frac) * lingam + frac * ls, ls)
    return ls


def clip_classes(w, lin):
    """EMPTY / PLAIN / PLAIN_LIN of the clips that have no highlight branch."""
    return np.where(w <= 0, EMPTY, np.where(w < _s(lin), PLAIN_LIN, PLAIN))


def plainclip(buf, gam_m_1, lin, lingam, brightness):
    p = _buf(buf)
    w = p[:, 3]
    live = w > 0
    out = np.zeros_like(p)
    out[live] = p[live] * (_clip_ls(w[live], _s(gam_m_1), _s(lin), _s(lingam)) * _s(brightness))[:, None]
    return out


def colorclip(buf, vib, highpow, gam, lin, lingam):
    """Returns (out, classes): the clipped buffer and the branch class of every pixel (EMPTY .. PLAIN_LIN)."""
    vib, highpow, gam, lin, lingam = _s(vib), _s(highpow), _s(gam), _s(lin), _s(lingam)
    p = _buf(buf)
    n = p.shape[0]
    w = p[:, 3]
    live = w > 0
    ws = np.where(live, w, 1.0)
    alpha = ws ** gam
    below = live & (w < lin)
    if lin > 0:
        frac = ws / lin
        alpha = np.where(below, (1.0 - frac) * ws * lingam + frac * alpha, alpha)
    ls = vib * alpha / ws
    alpha = np.clip(alpha, 0.0, 1.0)
    c = p[:, :3]
    maxc = c.max(1)
    maxa = maxc * ls
    hot = live & (maxa > 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        newls = 1.0 / maxc
        if highpow >= 0:
            lsratio = (newls / ls) ** highpow
            high = maxc[:, None] - (maxc[:, None] - c * newls[:, None]) * lsratio[:, None]
            cls = np.where(hot, HIGHLIGHT, PLAIN)
        else:
            high = None
            cls = np.where(hot & (-highpow < 1.0), BLENDED, PLAIN)
        adjhlp = np.where((-highpow > 1.0) | (maxa <= 1.0), 1.0, -highpow)
        adj = np.where(maxc > 0, (1.0 - adjhlp) * np.where(maxc > 0, newls, 0.0) + adjhlp * ls, 1.0)
    rgb = c * adj[:, None]
    if high is not None:
        rgb = np.where(hot[:, None], high, rgb)
    rgb = np.minimum(1.0, rgb + (1.0 - vib) * c ** gam)
    out = np.zeros((n, 4))
    out[live, :3] = rgb[live]
    out[live, 3] = alpha[live]
    cls = np.where(live, cls + np.where(below, 3, 0), EMPTY)
    return out, cls


def logencode(buf, degamma):
    """log2(x^degamma) / 12 + 1 per channel; -inf at x == 0."""
    p = _buf(buf)
    with np.errstate(divide='ignore'):
        return np.log2(p ** _s(degamma)) * (1.0 / 12.0) + 1.0


def _shear_blur(img, H, W, pattern, coefs):
    """7 taps along a shear pattern at offsets rint(pat * (i - 3)) (nearest-even, taken per component before it is added to the
    pixel position), addresses clamped to the buffer (cuburn/code/filters.py:22-35, :120-151).  img: (H * W, C)."""
    px, py = PATTERNS[pattern]
    src = img.reshape(H, W, -1)
    out = np.zeros_like(src)
    for i in range(7):
        dx, dy = int(np.rint(px * (i - 3))), int(np.rint(py * (i - 3)))
        ys = np.clip(np.arange(H) + dy, 0, H - 1)
        xs = np.clip(np.arange(W) + dx, 0, W - 1)
        out += src[np.ix_(ys, xs)] * coefs[i]
    return out.reshape(img.shape)


def smearclip_chain(buf, ah, astride, width, gam_m_1, lin, lingam):
    """gamma_full_hi (what of each pixel lies above density 1), blurred along patterns 2, 3, 0, 1 with a gaussian of `width`,
    added back, then the plain gamma clip.  Returns (out, classes), classes by the density after the smear is added."""
    p = _buf(buf)
    assert p.shape[0] == ah * astride
    w = p[:, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        ls = np.where(w > 0, np.maximum(0.0, w - 1.0) / w, 0.0)
    smear = p * ls[:, None]
    k = gauss_coefs(width)
    for pattern in (2, 3, 0, 1):
        smear = _shear_blur(smear, ah, astride, pattern, k)
    p = p + smear
    w = p[:, 3]
    live = w > 0
    out = np.zeros_like(p)
    out[live] = p[live] * _clip_ls(w[live], _s(gam_m_1), _s(lin), _s(lingam))[:, None]
    return out, clip_classes(w, lin)


def haloclip_chain(buf, ah, astride, gam_m_1):
    """pix.x^0.1 (the FIRST channel, cuburn/code/filters.py:270-271), blurred along patterns 2 and 3 with a unit gaussian, divides
    w^(gam - 1) where it is above 1.  Returns (out, classes)."""
    p = _buf(buf)
    assert p.shape[0] == ah * astride
    den = (p[:, 0] ** _s(0.1))[:, None]
    k = gauss_coefs(1.0)
    for pattern in (2, 3):
        den = _shear_blur(den, ah, astride, pattern, k)
    w = p[:, 3]
    live = w > 0
    out = np.zeros_like(p)
    out[live] = p[live] * (w[live] ** _s(gam_m_1) / np.maximum(1.0, den[live, 0]))[:, None]
    return out, np.where(live, PLAIN, EMPTY)
