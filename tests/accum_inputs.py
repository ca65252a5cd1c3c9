"""Synthetic accumulation buffers for the filter tests and tools/ (numpy only)."""
import numpy as np


def synth_accum(dim, seed=1):
    """A plausible accumulation buffer: smooth blobs + sparse noise + empty regions, YUV-ish."""
    rs = np.random.RandomState(seed)
    H, W = dim.ah, dim.astride
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    dens = np.zeros((H, W), np.float32)
    for _ in range(6):
        cx, cy, s = rs.uniform(0, W), rs.uniform(0, H), rs.uniform(8, 60)
        dens += rs.uniform(20, 2000) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    dens = rs.poisson(dens).astype(np.float32)
    dens[: H // 5] = 0
    buf = np.zeros((H, W, 4), np.float32)
    buf[..., 3] = dens
    buf[..., 0] = dens * rs.uniform(0.1, 0.9, (H, W))
    buf[..., 1] = dens * rs.uniform(0.3, 0.7, (H, W))
    buf[..., 2] = dens * rs.uniform(0.3, 0.7, (H, W))
    return buf.reshape(-1, 4)


def sparse_accum(dim, seed=3):
    """A few-samples-per-pixel buffer: isolated single hits, empty gaps, black and saturated colours
    (the regime where the DE weights underflow to denormals)."""
    rs = np.random.RandomState(seed)
    H, W = dim.ah, dim.astride
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    lam = 0.02 + 3.0 * np.exp(-((xx - W * 0.6) ** 2 + (yy - H * 0.5) ** 2) / (2 * 25.0 ** 2))
    lam[:, : W // 4] = 0.002
    dens = rs.poisson(lam).astype(np.float32)
    dens[H // 2, W // 8] = 900.0                      # one bright pixel in the empty quarter
    col = rs.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(H, W, 3))
    buf = np.zeros((H, W, 4), np.float32)
    buf[..., 3] = dens
    buf[..., :3] = dens[..., None] * col
    return buf.reshape(-1, 4)


def fractional_band_accum(dim, seed=1):
    """The parity tests' accumulator (blobs + Poisson + an empty band), with a band of fractional densities, many
    of them in (0, 1)."""
    buf = synth_accum(dim, seed).reshape(dim.ah, dim.astride, 4)
    r0 = dim.ah // 5                                        # rows above are empty
    buf[r0:r0 + 24] *= np.float32(0.37)
    rs = np.random.RandomState(seed)
    buf[r0 - 6:r0 - 2, 20:120, 3] = rs.uniform(0.05, 0.95, (4, 100)).astype(np.float32)
    buf[r0 - 6:r0 - 2, 20:120, :3] = buf[r0 - 6:r0 - 2, 20:120, 3:] * rs.uniform(0.2, 0.8, (4, 100, 3)).astype(np.float32)
    w = buf[r0 - 8:r0 + 24, :, 3]
    assert (w == 0).any() and ((w > 0) & (w < 1)).any() and (w % 1 != 0).any()
    return buf
