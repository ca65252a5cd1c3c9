"""
Model of xform chaos (flam3 xaos) as the contract states it: include/flame_hip.h (5) "Contract of a chaos kernel" and (6)
FL_OP_CHAOS_CDF; DESIGN.md §4.1 "Xaos".  The CPU oracle knows nothing of chaos; this is numpy.

  * the op in float64 (`cdf64`) and restated in float32 in the kernel's order of operations (`cdf32`), vectorised over the
    temporal samples: weights (S, n), chaos entries (S, n, n) -> cumulative rows (S, n, n);
  * the exact pair masses of a table: M_pn is row p as differences of the float64 rows, pi its stationary vector, the mass of
    the pair (p -> n) is pi_p M_pn; `lambda2` is the second-largest eigenvalue modulus of M, which bounds the chain's
    autocorrelation;
  * a per-sample Markov chaos game on affine boxes, vectorised over walkers, in the contract's order: a reseeded walker picks
    its xform from the plain row, every round applies xform p = next, then draws next from row p.

And the test flame: three `linear` xforms, xform k maps [-1, 1]^2 onto the square of side 1/2 at its own centre, centres chosen
so that the nine second-level boxes A_n(A_p(square)) — squares of side 1/8 at c_n + c_p / 4 — have disjoint closures: a sample
plotted in box (p, n) was produced by n after p, so the picture shows the transition counts.
"""
import copy

import numpy as np

F32 = np.float32
CENTRES = ((-0.6, -0.6), (0.6, -0.6), (0.0, 0.6))
WEIGHTS = (0.5, 0.3, 0.2)
SIDE = 0.25                    # xform k: x -> c_k + SIDE * x
PX_PER_UNIT = 128.0            # the test camera at 256 x 256


# ------------------------------------------------------------------ the op
def cdf64(w, c):
    w, c = np.asarray(w, np.float64), np.asarray(c, np.float64)
    d = w[:, None, :] * np.maximum(c, 0.0)
    plain = ~(d.sum(-1) > 0.0)
    d = np.where(plain[..., None], w[:, None, :] * np.ones_like(c), d)
    o = np.cumsum(d * (1.0 / d.sum(-1))[..., None], -1)
    o[..., -1] = 2.0
    return o


def cdf32(w, c):
    """csrc/interp.hip, case FL_OP_CHAOS_CDF, operation by operation in float32 (no contraction)."""
    w, c = np.asarray(w, F32), np.asarray(c, F32)
    S, n = w.shape
    out = np.zeros((S, n, n), F32)
    for p in range(n):
        cc = np.maximum(c[:, p, :], F32(0))
        total = np.zeros(S, F32)
        for k in range(n):
            total = total + w[:, k] * cc[:, k]
        plain = ~(total > 0)
        plain_total = np.zeros(S, F32)
        for k in range(n):
            plain_total = plain_total + w[:, k]
        total = np.where(plain, plain_total, total)
        with np.errstate(divide='ignore', invalid='ignore'):
            rsum = F32(1) / total
        run = np.zeros(S, F32)
        for k in range(n):
            run = run + np.where(plain, w[:, k], w[:, k] * cc[:, k]) * rsum
            out[:, p, k] = run
        out[:, p, n - 1] = F32(2)
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------ the chain
def transition(rows):
    """(n, n) cumulative rows -> the transition matrix M (rows sum to 1: the last word takes what is left)."""
    r = np.array(rows, np.float64)
    r[:, -1] = 1.0
    return np.diff(np.concatenate([np.zeros((len(r), 1)), r], 1), axis=1)


def stationary(M):
    vals, vecs = np.linalg.eig(M.T)
    v = np.real(vecs[:, np.argmin(np.abs(vals - 1.0))])
    return v / v.sum()


def lambda2(M):
    return float(np.sort(np.abs(np.linalg.eigvals(M)))[-2])


def pair_masses(M):
    return stationary(M)[:, None] * M


def sigma(N, r, lam):
    """Standard deviation of the count of a box of exact mass r among N samples of chains whose autocorrelation decays at
    least as fast as lam^k: the binomial's, widened by (1 + lam) / (1 - lam).  Derived, not measured."""
    return np.sqrt(N * r * (1.0 - r) * (1.0 + lam) / (1.0 - lam))


# ------------------------------------------------------------------ the test flame
def nine_boxes(chaos=None, samples=2 ** 24, weights=WEIGHTS, size=256):
    """(genome, profile).  ``chaos``: None, or a 3 x 3 table whose entries are numbers, splines, or None (no entry)."""
    from cuburn_amd import configs
    xforms = {}
    for k, ((ox, oy), w) in enumerate(zip(CENTRES, weights)):
        xforms[str(k)] = {'weight': w, 'color': 0.5 * k, 'color_speed': 0.5,
                          'pre_affine': configs._affine(0, SIDE, ox, oy), 'variations': {'linear': {'weight': 1.0}}}
        if chaos is not None:
            tab = dict((str(n), copy.deepcopy(v)) for n, v in enumerate(chaos[k]) if v is not None)
            if tab:
                xforms[str(k)]['chaos'] = tab
    gnm = {'type': 'animation', 'name': 'nine-boxes',
           'camera': {'center': {'x': 0.0, 'y': 0.0}, 'rotation': 0.0, 'scale': PX_PER_UNIT / size},
           'time': {'duration': 1, 'frame_width': 0.0},
           'palette': [configs._pal(0.0, configs.grey_ramp())], 'xforms': xforms}
    prof = {'width': size, 'height': size, 'spp': samples / float(size * size), 'fps': 1, 'duration': 1, 'frame_width': 0,
            'output': {'type': 'raw'}, 'filter_order': ['bilateral', 'logscale', 'colorclip']}
    return gnm, prof


def affines_of(block, prog):
    """Camera and pre affines (2 x 3 each) of the selectable xforms, from one parameter block."""
    cam = np.asarray(block[0:6], np.float64).reshape(2, 3)
    xo, xs = int(prog[5]), int(prog[6])
    return cam, [np.asarray(block[xo + i * xs: xo + i * xs + 6], np.float64).reshape(2, 3) for i in range(int(prog[1]))]


def _apply(a, pts):
    return pts @ a[:, :2].T + a[:, 2]


def box_rects(cam, aff, margin=1):
    """Pixel rectangles (r0, r1, c0, c1; inclusive) of the first-level boxes [k] and the second-level boxes [(p, n)] =
    camera(A_n(A_p([-1, 1]^2))), a pixel of margin around each."""
    sq = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])

    def rect(pts):
        px = _apply(cam, pts)
        return (int(np.floor(px[:, 1].min())) - margin, int(np.ceil(px[:, 1].max())) + margin,
                int(np.floor(px[:, 0].min())) - margin, int(np.ceil(px[:, 0].max())) + margin)
    first = [rect(_apply(a, sq)) for a in aff]
    second = dict(((p, n), rect(_apply(aff[n], _apply(aff[p], sq)))) for p in range(len(aff)) for n in range(len(aff)))
    return first, second


def rect_gap(a, b):
    """Pixels between two rectangles (Chebyshev; <= 0: they touch or overlap)."""
    return max(a[0] - b[1], b[0] - a[1], a[2] - b[3], b[2] - a[3]) - 1


def in_rect(img, rect):
    r0, r1, c0, c1 = rect
    return img[r0:r1 + 1, c0:c1 + 1]


def chaos_game(cam, aff, plain_row, rows, nwalkers, nrounds, fuse, dim, seed=1):
    """The contract's walk on affine xforms: a histogram (dim = rows, columns) of the samples of the write-enabled rounds."""
    rng = np.random.default_rng(seed)
    n = len(aff)
    pick = lambda row, u: np.minimum(np.searchsorted(row[:n - 1], u, side='left'), n - 1)      # the smallest k with u <= row[k], else n - 1
    pts = rng.uniform(-1.0, 1.0, (nwalkers, 2))
    nxt = pick(np.asarray(plain_row, np.float64), rng.uniform(0.0, 1.0, nwalkers))
    rows = np.asarray(rows, np.float64)
    hist = np.zeros(dim[0] * dim[1], np.int64)
    for r in range(fuse + nrounds):
        new, new_next = np.empty_like(pts), np.empty_like(nxt)
        u = rng.uniform(0.0, 1.0, nwalkers)
        for p in range(n):
            m = nxt == p
            new[m] = _apply(aff[p], pts[m])
            new_next[m] = pick(rows[p], u[m])
        pts, nxt = new, new_next
        if r >= fuse:
            px = np.rint(_apply(cam, pts)).astype(np.int64)
            ok = (px[:, 0] >= 0) & (px[:, 0] < dim[1]) & (px[:, 1] >= 0) & (px[:, 1] < dim[0])
            hist += np.bincount(px[ok, 1] * dim[1] + px[ok, 0], minlength=hist.size)
    return hist.reshape(dim)
