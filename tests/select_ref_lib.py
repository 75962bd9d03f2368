"""The selection rule of rtpbr_select_noisy (include/rtpbr.h) in numpy.  Comparisons only, so this restatement is exact.

    select(noise, count, threshold, dilate) -> (W,H) uint8

Pixel p is selected when ``count[p] > 0`` is false (no samples), or some pixel q inside the frame with
max(|dx|, |dy|) <= dilate has ``noise[q] > threshold``.  ``ordered_list(mask)`` is the list the library builds from a mask:
the selected buffer indices x * H + y in ascending order."""
import numpy as np


def select(noise, count, threshold, dilate=0):
    noise = np.asarray(noise, np.float32)
    count = np.asarray(count, np.float32)
    if noise.ndim != 2 or noise.shape != count.shape:
        raise ValueError("noise and count must be (W,H) arrays of one shape")
    if not 0 <= int(dilate) <= 3:
        raise ValueError("dilate must be 0..3")
    if not np.float32(threshold) >= 0:
        raise ValueError("threshold must be >= 0")
    d = int(dilate)
    W, H = noise.shape
    above = noise > np.float32(threshold)              # NaN compares false, as on the device
    near = np.zeros((W, H), bool)
    for dx in range(-d, d + 1):
        for dy in range(-d, d + 1):
            # near[x, y] |= above[x + dx, y + dy] where that lies inside the frame
            xs, xe = max(0, -dx), min(W, W - dx)
            ys, ye = max(0, -dy), min(H, H - dy)
            if xs < xe and ys < ye:
                near[xs:xe, ys:ye] |= above[xs + dx:xe + dx, ys + dy:ye + dy]
    return (near | ~(count > 0)).astype(np.uint8)


def ordered_list(mask):
    return np.flatnonzero(np.asarray(mask).reshape(-1) != 0).astype(np.uint32)
