"""numpy restatement of rtpbr_present (include/rtpbr.h): a (W,H,3) float32 field — [x][y], y = 0 at the bottom — becomes the
(H,W,C) uint8 frame, top row first.  Every operation is float32, in the header's order: NaN -> 0, clamp to [0,1], one rounded
multiply by 255, one rounded add of t, truncation.  The GPU tests hold the kernel to this and to nothing else."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE_PIXELS, SOURCE_DENOISED, SOURCE_ACCUM = 0, 1, 2
FORMAT_RGB8, FORMAT_RGBA8 = 0, 1

BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                  [48, 16, 56, 24, 50, 18, 58, 26],
                  [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22],
                  [3, 35, 11, 43, 1, 33, 9, 41],
                  [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37],
                  [63, 31, 55, 23, 61, 29, 53, 21]], np.uint8)

F = np.float32


def thresholds(w, h, dither):
    """t of every frame element, (H, W, 1) float32: row = the top-down row r, column = x"""
    if not dither:
        return np.full((h, w, 1), 0.5, F)
    r, x = np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7
    return ((BAYER[r, x].astype(F) + F(0.5)) * F(0.015625))[..., None]


def present(field, fmt=FORMAT_RGBA8, dither=False):
    """field (W,H,3) float32 -> (H,W,3|4) uint8"""
    a = np.asarray(field)
    assert a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 3
    w, h = a.shape[:2]
    v = np.swapaxes(a, 0, 1)[::-1]                      # [r][x][c] = field[x][H - 1 - r][c]
    v = np.where(v != v, F(0), v)
    v = np.minimum(np.maximum(v, F(0)), F(1))
    p = v * F(255.0)                                     # rounded to float32 here ...
    assert p.dtype == np.float32
    q = (p + thresholds(w, h, dither)).astype(np.uint8)  # ... and again after the add; the conversion truncates
    if fmt == FORMAT_RGBA8:
        q = np.concatenate([q, np.full((h, w, 1), 255, np.uint8)], -1)
    return np.ascontiguousarray(q)
