"""Call sequences over rtpbr_blend_error / rtpbr_select_blend_error: the generator and the state model of tests/half_sequences.py
and tests/half_mode_model.py (both unchanged) with draws for the two calls between samples, selected samples, half updates,
reprojections, refreshes and new resolutions, and the lock-step driver for them.

``BlendErrorState`` adds the refusal rules of include/rtpbr.h for the two calls; ``BlendErrorModel.apply(op)`` returns what
HalfModel.apply returns, with ``blend_error_map``, ``denoised_pixels``, ``blend_weight`` and ``blend_depth`` among the expected
values wherever rtpbr_blend_error writes them (tests/blend_error_ref_lib.py on the model's own image_buffer, half A and features).
Readings of the header this model fixes: the error plane comes into being with the first rtpbr_blend_error that is not refused and
goes with a new resolution; rtpbr_select_blend_error reads it as that call left it, whatever has been sampled since; neither call
touches RTPBR_BUF_DENOISED_ERROR, and rtpbr_denoise_error does not touch the new plane."""
import numpy as np

import blend_error_ref_lib as be
import call_sequences as cs
import half_mode_model as hmm
import half_ref_lib as hl
import half_sequences as hs
import post_model as pm
from raytracingpbr_amd._capi import RtpbrError

EINVAL, ESTATE, MISSING = cs.EINVAL, cs.ESTATE, pm.MISSING
KINDS = ("blend_error", "select_blend_error")
BLENDS = (None, (1, 0.0, 1), (2, 0.0, 2), (3, 2.0, 1), (2, 0.5, 16777216))      # (radius, z, min_half_samples); None: NULL
BAD_BLENDS = ((0, 2.0, 16), (4, 2.0, 16), (3, -1.0, 16), (3, 2.0, 0))


class Op(hs.Op):
    def code(self):
        a, k = self.args, self.kind
        if k == "blend_error":
            b = a["blend"] or (None, None, None)
            return f"r.blend_error({a['threshold']}, {b[0]}, {b[1]}, {b[2]}, {a['window']}, **{a['params']!r})"
        if k == "select_blend_error":
            return f"r.select_blend_error({a['threshold']}, {a['dilate']})"
        return super().code()


class BlendErrorState(hmm.HalfState):
    """HalfState and the two calls; ``exists`` also keeps "blend_error_map" """

    def models(self, op):
        return super().models(op) or op.kind in KINDS

    def bad(self, op):
        a, k = op.args, op.kind
        if k == "blend_error":
            r, z, m = a["blend"] or (3, 2.0, 16)
            p = a["params"]
            ok = (a["window"] is None or 1 <= a["window"] <= 3) and a["threshold"] >= 0 and 1 <= r <= 3 and 0 <= z < float("inf") \
                and 1 <= m <= 16777216 and 0 <= p.get("iterations", 4) <= 8 and p.get("demodulate", 0) in (0, 1)
            return None if ok else "argument"
        if k == "select_blend_error":
            return None if a["threshold"] >= 0 and 0 <= a["dilate"] <= 3 else "argument"
        return super().bad(op)

    def state_reasons(self, op):
        k, why = op.kind, super().state_reasons(op)
        if k in KINDS and self.tiles[3] > 1:
            why.append("tiles")
        if k == "blend_error" and "half_buffer" not in self.exists:
            why.append("no_halves")
        if k == "select_blend_error" and not {"half_buffer", "blend_error_map"} <= self.exists:
            why.append("no_blend_error")
        return why

    def note(self, op):
        super().note(op)                            # (a new resolution empties ``exists`` first)
        if op.kind == "blend_error":
            self.exists |= {"blend_error_map", "denoised_pixels"}
            self.denoised_by = "denoise"
        elif op.kind == "select_blend_error":
            self.exists.add("selection")
            self.selected = True


class BlendErrorModel(hmm.HalfModel):
    """HalfModel with the last error plane of the blended frame, its weight and its depth"""
    STATE = BlendErrorState

    def __init__(self, s, threads=0):
        super().__init__(s, threads)
        self.blend = None                    # the last BlendError, once there is one

    def apply(self, op):
        size = self._size()
        res = super().apply(op)
        if res[0] is None and self._size() != size:
            self.blend = None
        return res

    def _observe(self, what):
        want = super()._observe(what)
        if what == "post":
            b = self.blend
            want["blend_error_map"] = MISSING if b is None else b.error
            if b is not None:                # (the weight exists from rtpbr_denoise_blend on as well, which no draw calls)
                want["blend_weight"], want["blend_depth"] = b.weight, b.depth
        return want

    def _do_blend_error(self, op):
        a = op.args
        r, z, m = a["blend"] or (None, None, None)
        b = be.blend_error(self.st.cfg, self.o.image_buffer, self.halves.a, self._features(), a["threshold"], r, z, m, a["window"],
                           **a["params"])
        self.blend = b
        self.last["denoised_pixels"] = b.denoised
        usable = int((b.weight < 1).sum())
        self.events.append(("blend_error", b.stats[0], b.error.size, usable, bool((b.bias2 > 0).any())))
        return {"blend_error_map": b.error, "denoised_pixels": b.denoised, "blend_weight": b.weight, "blend_depth": b.depth,
                "stats": (b.stats[0], b.stats[1], int(np.float32(b.stats[2]).view(np.uint32)))}

    def _do_select_blend_error(self, op):
        a = op.args
        self.mask = hl.select(self.o.image_buffer, self.halves.a, self.blend.error, a["threshold"], a["dilate"], self.st.estimator[2])
        self.events.append(("select_blend_error", int(self.mask.sum()), self.mask.size))
        return {"selection": self.mask, "n_selected": int(self.mask.sum())}


class _Grammar(hs._Grammar):
    def new(self, kind, **args):
        op = Op(kind, **args)
        op.expect, why = self.m.refusal(op)
        op.why = tuple(why)
        return self.add(op)

    def blend_error(self, **over):
        a = dict(threshold=float(self.pick(cs.THRESHOLDS)), window=self.pick((None, 1, 2, 3)), blend=self.pick(BLENDS),
                 params=dict(self.pick(hs.DENOISE)))
        a.update(over)
        return self.new("blend_error", **a)

    def select_blend_error(self):
        return self.new("select_blend_error", threshold=float(self.pick(cs.THRESHOLDS)), dilate=int(self.rng.integers(0, 4)))

    def blend_op(self):
        """one draw of the two calls (one or a few operations)"""
        rng, pick, m, add, new = self.rng, self.pick, self.m, self.add, self.new
        u = rng.random()
        if u < 0.45:                                                        # rounds of the loop on batches dealt by half_update
            self.whole_frame(0.9)
            if "half_buffer" not in m.exists or rng.random() < 0.6:
                self.two_batches()
            for _ in range(int(pick((1, 1, 2)))):
                if self.blend_error().expect is None and rng.random() < 0.8:
                    if self.select_blend_error().expect is None:
                        new("sample_selected", n=self.tracked_n())
                        if rng.random() < 0.7:
                            new("half_update")
            if rng.random() < 0.5:
                add(Op("observe", what="post"))
        elif u < 0.6:                                                       # the selection reads the plane as it was left
            self.whole_frame(0.9)
            self.sample(self.spp())
            new("half_update")
            if rng.random() < 0.5:
                self.error()                                                # (rtpbr_denoise_error writes a plane of its own)
            self.select_blend_error()
            add(Op("observe", what="post"))
        elif u < 0.75:                                                      # after a reprojection: empty halves, pixels without samples
            self.history()
            if "half_buffer" not in m.exists:
                self.two_batches()
            if self.reproject().expect is None:
                if rng.random() < 0.6:
                    self.sample(self.spp())
                    new("half_update")
                self.blend_error()
                self.select_blend_error()
        elif u < 0.87:                                                      # refresh and a new resolution
            if rng.random() < 0.5:
                add(Op("refresh"))
            else:
                w, h = pick([s for s in self.sizes if s != (m.cfg.width, m.cfg.height)])
                self.set_config(width=w, height=h)
                self.select_blend_error()                                   # RTPBR_ESTATE: the plane went with the resolution
            self.whole_frame(0.9)
            self.blend_error()
            self.two_batches()
            self.blend_error()
        else:                                                               # the calls' own refusals
            self.whole_frame(1.0)
            probe = Op("blend_error", threshold=0.0, window=None, blend=None, params={})
            if not m.state_reasons(probe) and self.clean():
                v = rng.random()
                if v < 0.35:
                    self.blend_error(threshold=float(pick((0.0, -1.0))), window=pick((0, 4)))
                elif v < 0.7:
                    self.blend_error(blend=pick(BAD_BLENDS))
                else:
                    self.blend_error(params={"iterations": 9})
                if not m.state_reasons(Op("select_blend_error", threshold=0.0, dilate=0)):
                    new("select_blend_error", threshold=0.02, dilate=int(pick((-1, 4))))
            else:
                self.blend_error()                                          # (before half A exists, or with tiles: RTPBR_ESTATE)
                new("select_blend_error", threshold=0.02, dilate=1)


def blend_script(seed, n_ops=30, jit=0, scenes=hs.SCENES, forms=(0,)):
    """A call sequence over rtpbr_blend_error: a third of the draws are those of half_sequences and its parents, the rest are
    blend_op()."""
    g = _Grammar(seed, scenes, forms, hs.SIZES, BlendErrorState)
    while len(g.ops) < n_ops:
        u = g.rng.random()
        if u < 0.1:
            g.old_op()
        elif u < 0.2:
            g.post_op()
        elif u < 0.35:
            g.half_op()
        else:
            g.blend_op()
    g.add(Op("observe", what="all"))
    g.add(Op("observe", what="post"))
    return cs.Script(seed, g.base, g.scene0, g.ops, jit, post=True, motion=True)


def model(s, threads=0):
    return BlendErrorModel(s, threads)


# ------------------------------------------------------------------ the driver
def _apply(op, r):
    """apply one operation to the HIP renderer; (code or None, {name: value} of what the call itself returned)"""
    a, k = op.args, op.kind
    try:
        if k == "blend_error":
            rd, z, m = a["blend"] or (None, None, None)
            st = r.blend_error(a["threshold"], rd, z, m, a["window"], **a["params"])
            return None, {"stats": (st.pixels_estimated, st.pixels_above, int(np.float32(st.max_noise).view(np.uint32)))}
        if k == "select_blend_error":
            return None, {"n_selected": r.select_blend_error(a["threshold"], a["dilate"])}
    except RtpbrError as e:
        return e.code, {}
    return hs._apply_half(op, r)


def run(s, hip, mdl, upto=None):
    """half_sequences.run_half for a blend_script: the HIP renderer `hip` (None: the model alone, its codes against the script's)
    and the BlendErrorModel `mdl` in lock step.  Raises call_sequences.Mismatch with a replayable report; returns the list of
    (operation index, name, expected value) and the model's events."""
    seen, last_ok_of = [], {}
    ops = s.ops if upto is None else s.ops[:upto]

    def fail(i, what, key=None):
        start = last_ok_of.get(key, -1)
        lines = [f"blend-error call sequence seed {s.seed}, operation #{i}: {what}", s.header(),
                 "operations since " + (f"{key} last matched" if key else "the start") + f" (#{start + 1}..#{i}):"]
        lines += [f"  [{j}] {s.ops[j]!r}" for j in range(start + 1, i + 1)]
        lines.append(f"replay: blend_error_sequences.replay(blend_error_sequences.blend_script({s.seed}, ...), upto={i + 1})")
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
    """rerun a blend_script (or its first `upto` operations) on a fresh HIP renderer against a fresh model"""
    from raytracingpbr_amd import Renderer
    a, b = cs.new_renderer(s, Renderer), model(s, threads)
    try:
        return run(s, a, b, upto)
    finally:
        a.close()
        b.close()
