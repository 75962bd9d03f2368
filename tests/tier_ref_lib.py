"""The tier rule of the select calls with option select_tiers = T (include/rtpbr.h) and the stage plan of a tiered
rtpbr_sample_selected, in numpy.  Float32 division, multiplication, subtraction and comparisons only: every numpy operation on
float32 arrays is one exactly rounded f32 operation, so this restatement is exact.

    select(plane, count, threshold, dilate, tiers, batch, min_samples=0, half_count=None) -> (W,H) uint8: 0 or 1 + tier
    mask(bytes, tiers)                                                                    -> (W,H) uint8: 0 or 1 + tier
    ordered_list(sel)      the list the library builds: tier ascending, ascending buffer index x * H + y within a tier
    counts(sel, tiers)     pixels per tier
    shares(n, tiers)       what sample_selected(n) gives a pixel of each tier
    stage_plan(n, counts)  the stages that run: (tier t, first index, end index, L_t) with the indices relative to sample_base
"""
import numpy as np

f32 = np.float32


def _window(a, d, combine, out):
    """out[x, y] = combine over the pixels (x + dx, y + dy) inside the frame, max(|dx|, |dy|) <= d, of a"""
    W, H = a.shape
    for dx in range(-d, d + 1):
        for dy in range(-d, d + 1):
            xs, xe = max(0, -dx), min(W, W - dx)
            ys, ye = max(0, -dy), min(H, H - dy)
            if xs < xe and ys < ye:
                out[xs:xe, ys:ye] = combine(out[xs:xe, ys:ye], a[xs + dx:xe + dx, ys + dy:ye + dy])
    return out


def bounds(tiers, batch):
    """(float)max(1, B >> k) for k = 1 .. T - 1"""
    return [f32(max(1, int(batch) >> k)) for k in range(1, int(tiers))]


def select(plane, count, threshold, dilate, tiers, batch, min_samples=0, half_count=None):
    plane, count = np.asarray(plane, f32), np.asarray(count, f32)
    if plane.ndim != 2 or plane.shape != count.shape:
        raise ValueError("plane and count must be (W,H) arrays of one shape")
    if not 0 <= int(dilate) <= 3:
        raise ValueError("dilate must be 0..3")
    if not f32(threshold) >= 0:
        raise ValueError("threshold must be >= 0")
    if not 1 <= int(tiers) <= 8 or not 1 <= int(batch) <= 65536:
        raise ValueError("tiers must be 1..8, batch 1..65536")
    thr, d = f32(threshold), int(dilate)
    # selected whatever the plane says: no samples, fewer than min_samples, (the error rules) an empty half
    young = ~(count > 0) | (count < f32(min_samples))
    if half_count is not None:
        ca = np.asarray(half_count, f32)
        with np.errstate(invalid="ignore"):
            young |= ~(ca > 0) | ~(count - ca > 0)
    above = plane > thr                                # NaN compares false, as on the device
    # every value that counts is > threshold >= 0, so 0 stands for "none"; no NaN gets in, so np.maximum is fmaxf
    m = _window(np.where(above, plane, f32(0)), d, np.maximum, np.zeros(plane.shape, f32))
    near = m > 0
    with np.errstate(all="ignore"):
        r = m / thr
        need = count * (r * r - f32(1))
    assert r.dtype == f32 and need.dtype == f32
    t = np.zeros(plane.shape, np.uint8)
    for b in bounds(tiers, batch):
        t += need <= b                                 # NaN and infinity: false
    return np.where(young, 1, np.where(near, 1 + t, 0)).astype(np.uint8)


def mask(raw, tiers):
    raw = np.asarray(raw)
    if raw.dtype != np.uint8:
        raise ValueError("a tier mask is uint8")
    return np.minimum(raw, np.uint8(tiers))


def ordered_list(sel):
    flat = np.asarray(sel).reshape(-1)
    tiers = int(flat.max()) if flat.size else 0
    return np.concatenate([np.flatnonzero(flat == 1 + t) for t in range(tiers)] + [np.zeros(0, np.int64)]).astype(np.uint32)


def counts(sel, tiers):
    flat = np.asarray(sel).reshape(-1)
    return tuple(int((flat == 1 + t).sum()) for t in range(int(tiers)))


def shares(n, tiers):
    return tuple(max(1, int(n) >> t) if n >= 1 else 0 for t in range(int(tiers)))


def stage_plan(n, tier_counts):
    """Stages t = T-1 .. 0: stage t traces the indices s_{t+1} .. s_t - 1 (s_T = 0) through the first L_t entries of the list;
    stages with no indices or no pixels are left out."""
    T = len(tier_counts)
    s = shares(n, T) + (0,)
    cum = np.cumsum(tier_counts).tolist()
    return [(t, s[t + 1], s[t], cum[t]) for t in range(T - 1, -1, -1) if s[t] != s[t + 1] and cum[t] > 0]


def traced(n, tier_counts):
    return sum(c * s for c, s in zip(tier_counts, shares(n, len(tier_counts))))
