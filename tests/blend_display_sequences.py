"""Call sequences over rtpbr_blend_error_display beside rtpbr_blend_error / rtpbr_select_blend_error: the generator, state model
and driver of tests/blend_error_sequences.py (unchanged) with one more kind, "blend_error_display", that every draw of an
estimate takes half the time.

Readings of the header this model fixes: the two estimate calls share RTPBR_BUF_BLEND_ERROR and nothing else tells them apart —
the same refusals, the same frame, weight and depth —; the plane holds what the LAST of the two wrote, comes into being with
either and goes with a new resolution; rtpbr_select_blend_error reads it whichever call left it."""
import numpy as np

import blend_error_ref_lib as be
import blend_error_sequences as bs
import call_sequences as cs
import half_sequences as hs
from raytracingpbr_amd._capi import RtpbrError

EINVAL, ESTATE = bs.EINVAL, bs.ESTATE
DISPLAY = "blend_error_display"


def _as_linear(op):
    """the rtpbr_blend_error with the same arguments: the two calls are refused alike"""
    return bs.Op("blend_error", **op.args)


class Op(bs.Op):
    def code(self):
        if self.kind == DISPLAY:
            a = self.args
            b = a["blend"] or (None, None, None)
            return f"r.blend_error({a['threshold']}, {b[0]}, {b[1]}, {b[2]}, {a['window']}, bias='display', **{a['params']!r})"
        return super().code()


class BlendDisplayState(bs.BlendErrorState):
    def models(self, op):
        return super().models(op) or op.kind == DISPLAY

    def bad(self, op):
        return super().bad(_as_linear(op) if op.kind == DISPLAY else op)

    def state_reasons(self, op):
        return super().state_reasons(_as_linear(op) if op.kind == DISPLAY else op)

    def note(self, op):
        super().note(_as_linear(op) if op.kind == DISPLAY else op)


class BlendDisplayModel(bs.BlendErrorModel):
    STATE = BlendDisplayState

    def _do_blend_error(self, op, display=False):
        a = op.args
        r, z, m = a["blend"] or (None, None, None)
        b = be.blend_error(self.st.cfg, self.o.image_buffer, self.halves.a, self._features(), a["threshold"], r, z, m, a["window"],
                           display=display, **a["params"])
        self.blend = b
        self.last["denoised_pixels"] = b.denoised
        self.events.append((op.kind, b.stats[0], b.error.size, int((b.weight < 1).sum()), bool((b.bias2 > 0).any())))
        return {"blend_error_map": b.error, "denoised_pixels": b.denoised, "blend_weight": b.weight, "blend_depth": b.depth,
                "stats": (b.stats[0], b.stats[1], int(np.float32(b.stats[2]).view(np.uint32)))}

    def _do_blend_error_display(self, op):
        return self._do_blend_error(op, display=True)


class _Grammar(bs._Grammar):
    def new(self, kind, **args):
        op = Op(kind, **args)
        op.expect, why = self.m.refusal(op)
        op.why = tuple(why)
        return self.add(op)

    def blend_error(self, **over):
        a = dict(threshold=float(self.pick(cs.THRESHOLDS)), window=self.pick((None, 1, 2, 3)), blend=self.pick(bs.BLENDS),
                 params=dict(self.pick(hs.DENOISE)))
        a.update(over)
        return self.new(DISPLAY if self.rng.random() < 0.5 else "blend_error", **a)


def display_script(seed, n_ops=30, jit=0, scenes=hs.SCENES, forms=(0,)):
    """blend_error_sequences.blend_script with every estimate one of the two calls, and in a fifth of the draws the pair on one
    state: the second restores its own rule's plane whatever the first left."""
    g = _Grammar(seed, scenes, forms, hs.SIZES, BlendDisplayState)
    while len(g.ops) < n_ops:
        u = g.rng.random()
        if u < 0.1:
            g.old_op()
        elif u < 0.2:
            g.post_op()
        elif u < 0.3:
            g.half_op()
        elif u < 0.5:
            g.whole_frame(0.9)
            if "half_buffer" not in g.m.exists:
                g.two_batches()
            # (levels and min_half_samples 1: wherever both halves hold samples there is a bias term for the rules to differ in)
            a = dict(threshold=float(g.pick(cs.THRESHOLDS)), window=g.pick((1, 2, 3)), blend=(g.pick((1, 2, 3)), g.pick((0.0, 2.0)), 1),
                     params={"iterations": g.pick((1, 2, 4)), "demodulate": g.pick((0, 1))})
            first = g.pick((DISPLAY, "blend_error"))
            g.new(first, **a)
            g.select_blend_error()
            g.new("blend_error" if first == DISPLAY else DISPLAY, **a)
            g.add(Op("observe", what="post"))
        else:
            g.blend_op()
    g.add(Op("observe", what="all"))
    g.add(Op("observe", what="post"))
    return cs.Script(seed, g.base, g.scene0, g.ops, jit, post=True, motion=True)


def model(s, threads=0):
    return BlendDisplayModel(s, threads)


def _apply(op, r):
    if op.kind == DISPLAY:
        a = op.args
        rd, z, m = a["blend"] or (None, None, None)
        try:
            st = r.blend_error(a["threshold"], rd, z, m, a["window"], bias="display", **a["params"])
        except RtpbrError as e:
            return e.code, {}
        return None, {"stats": (st.pixels_estimated, st.pixels_above, int(np.float32(st.max_noise).view(np.uint32)))}
    return bs._apply(op, r)


def run(s, hip, mdl, upto=None):
    """blend_error_sequences.run for a display_script (its driver with this module's _apply)"""
    seen, last_ok_of = [], {}
    ops = s.ops if upto is None else s.ops[:upto]

    def fail(i, what, key=None):
        start = last_ok_of.get(key, -1)
        lines = [f"blend-display call sequence seed {s.seed}, operation #{i}: {what}", s.header(),
                 "operations since " + (f"{key} last matched" if key else "the start") + f" (#{start + 1}..#{i}):"]
        lines += [f"  [{j}] {s.ops[j]!r}" for j in range(start + 1, i + 1)]
        lines.append(f"replay: blend_display_sequences.replay(blend_display_sequences.display_script({s.seed}, ...), upto={i + 1})")
        raise cs.Mismatch("\n".join(lines))

    for i, op in enumerate(ops):
        want_code, want = mdl.apply(op)
        if want_code != op.expect:
            fail(i, f"{op.kind}: the model expects {want_code}, the script {op.expect}")
        got = {}
        if hip is not None:
            code, got = _apply(op, hip)
            if code != op.expect:
                fail(i, f"{op.kind} returned {code}, expected {op.expect}")
        for k, y in want.items():
            if hip is not None:
                d = cs._first_diff(got[k] if k in got else cs._read_post(hip, k), y)
                if d is not None:
                    fail(i, f"{k} differs from the model: {d}", k)
            seen.append((i, k, y))
            last_ok_of[k] = i
    return seen, mdl.events


def replay(s, upto=None, threads=0):
    """rerun a display_script (or its first `upto` operations) on a fresh HIP renderer against a fresh model"""
    from raytracingpbr_amd import Renderer
    a, b = cs.new_renderer(s, Renderer), model(s, threads)
    try:
        return run(s, a, b, upto)
    finally:
        a.close()
        b.close()
