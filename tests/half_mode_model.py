"""The state model of rtpbr_set_half_mode for the call sequences of tests/half_sequences.py: post_model.MotionState and
post_model.MotionModel (unchanged) with what the two-half error estimate adds to a context — half A and its snapshot
(half_ref_lib.Halves), the last error map, and the mode.

``HalfState`` adds the refusal rules of include/rtpbr.h for rtpbr_set_half_mode, rtpbr_half_update, rtpbr_denoise_error and
rtpbr_select_error, and what the mode makes rtpbr_sample / rtpbr_sample_selected refuse.  ``HalfModel.apply(op)`` returns what
MotionModel.apply returns, with ``half_buffer`` / ``denoised_error`` among the expected values wherever a call writes them.

Readings of the header this model fixes.  A and sh come into being together (zeroed) with the first rtpbr_half_update, the set call
that turns per_sample from 0 to 1, or the first dealing sample call that is not refused — whatever n is, sample(0) and an empty
selection included; a refused one allocates nothing.  rtpbr_set_half_mode from 0 to 1 with tiles of world > 1 is rtpbr_half_update's
refusal and leaves BOTH fields as they were; every other transition succeeds in any state.  A dealing call takes the n colours of
every pixel from the model's own oracle exactly as MotionModel takes them for a tracked call (one draw serves both folds when both
modes are on) and deals them with half_mode_ref_lib.fold, whose image_buffer must be the oracle's.  A reprojection with warp on and
A present: half_mode_ref_lib.gather on the old A, whose image_buffer and motion must be the model's own; sh = the warped image.
With warp off, or for a written image_buffer: A = 0, sh = the new image_buffer; refresh: both 0; a new resolution: both gone, and
the error map with them.  A bad argument and a bad state together have no code in the header and are never drawn."""
import numpy as np

import call_sequences as cs
import checks as ck
import half_mode_ref_lib as hm
import half_ref_lib as hl
import post_model as pm

EINVAL, ESTATE, MISSING = cs.EINVAL, cs.ESTATE, pm.MISSING
HALF_KINDS = ("set_half_mode", "half_update", "denoise_error", "select_error")
DEALT = ("dealt:persistent", "dealt:tiles")


def mode_of(op):
    """(per_sample, warp) a set_half_mode operation asks for (mode None: the NULL pointer, the defaults)"""
    return (0, 0) if op.args["mode"] is None else tuple(op.args["mode"])


class HalfState(pm.MotionState):
    """MotionState and the half mode; ``exists`` also keeps "half_buffer" and "denoised_error" """

    def __init__(self, base, scene0):
        super().__init__(base, scene0)
        self.per_sample = False
        self.warp = False

    def models(self, op):
        return super().models(op) or op.kind in HALF_KINDS

    def bad(self, op):
        a, k = op.args, op.kind
        if k == "set_half_mode":
            return None if all(v in (0, 1) for v in mode_of(op)) else "argument"
        if k == "denoise_error":
            ok = (a["radius"] is None or 1 <= a["radius"] <= 3) and a["threshold"] >= 0
            return None if ok else "argument"
        if k == "select_error":
            return None if a["threshold"] >= 0 and 0 <= a["dilate"] <= 3 else "argument"
        return super().bad(op)

    def state_reasons(self, op):
        k, why = op.kind, super().state_reasons(op)
        tiled = self.tiles[3] > 1
        if k in ("half_update", "denoise_error", "select_error") and tiled:
            why.append("tiles")
        if k == "set_half_mode" and mode_of(op)[0] == 1 and not self.per_sample and tiled:      # what rtpbr_half_update refuses
            why.append("tiles")
        if k == "denoise_error" and "half_buffer" not in self.exists:
            why.append("no_halves")
        if k == "select_error" and not {"half_buffer", "denoised_error"} <= self.exists:
            why.append("no_error")
        if k in ("sample", "sample_selected") and self.per_sample:
            if k == "sample" and self.cfg.kernel_form != 0:
                why.append("dealt:persistent")
            if tiled:
                why.append("dealt:tiles")
        return why

    def stamp(self, op):
        """as MotionState.stamp: a sample operation that the mode refuses is stamped again, and one whose bad argument meets such
        a refusal is dropped"""
        op = super().stamp(op)
        if op is not None and op.kind == "sample" and self.per_sample:
            if [w for w in self.state_reasons(op) if w in DEALT]:
                if op.args["n"] < 0:
                    return None
                op.expect, op.why = ESTATE, tuple(self.state_reasons(op))
        return op

    def note(self, op):
        k = op.kind
        super().note(op)                            # (a new resolution empties ``exists`` first)
        if k in ("sample", "sample_selected") and self.per_sample:
            self.exists.add("half_buffer")
        elif k == "set_half_mode":
            ps, w = mode_of(op)
            if ps and not self.per_sample:
                self.exists.add("half_buffer")
            self.per_sample, self.warp = bool(ps), bool(w)
        elif k == "half_update":
            self.exists.add("half_buffer")
        elif k == "denoise_error":
            self.exists.add("denoised_error")
        elif k == "select_error":
            self.exists.add("selection")
            self.selected = True


class HalfModel(pm.MotionModel):
    """MotionModel with half A, its snapshot and the last error map"""
    STATE = HalfState

    def __init__(self, s, threads=0):
        super().__init__(s, threads)
        self.halves = None                   # half A + sh, once they exist
        self.error = None                    # RTPBR_BUF_DENOISED_ERROR, once it exists
        self.dealt = None                    # (colours, image_buffer before) of the dealing sample() that is being applied, tracking off

    def _halves(self):
        if self.halves is None:
            self.halves = hl.Halves(*self._size())
        return self.halves

    def apply(self, op):
        k, st = op.kind, self.st
        self.dealt = None
        if k == "sample" and st.per_sample:
            if [w for w in st.state_reasons(op) if w in DEALT]:
                return ESTATE, {}
            if not st.tracking and op.args["n"] >= 0 and (st.cfg.sky_kind != 1 or st.env):
                self.dealt = self._colours(op.args["n"])      # (with tracking on MotionModel.apply draws them)
        size = self._size()
        res = super().apply(op)
        if res[0] is None and self._size() != size:
            self.halves, self.error = None, None
        return res

    def _observe(self, what):
        want = super()._observe(what)
        if what == "post":
            want["half_buffer"] = MISSING if self.halves is None else self.halves.a.copy()
            want["denoised_error"] = MISSING if self.error is None else self.error
        return want

    # ------------------------------------------------------------ dealing
    def _deal(self, colours, before, mask):
        h = self._halves()
        if len(colours):
            A, s, b = hm.fold(colours, h.a, h.snapshot, before, mask)
            assert np.array_equal(ck.bits(b), ck.bits(self.o.image_buffer)), "the fold's image_buffer is not the call's without the mode"
            h.a[:], h.snapshot[:] = A, s
            n_sel = before.shape[0] * before.shape[1] if mask is None else int((np.asarray(mask) != 0).sum())
            self.events.append(("dealt", "sample" if mask is None else "sample_selected", len(colours), n_sel, self.st.tracking))
        return {"half_buffer": h.a.copy()}

    def _do_sample(self, op):
        out = super()._do_sample(op)
        c = self.colours if self.colours is not None else self.dealt
        if self.st.per_sample and c is not None:
            out = dict(out, image_buffer=self.o.image_buffer, **self._counters())
            out.update(self._deal(c[0], c[1], None))
        return out

    def _do_sample_selected(self, op):
        if not self.st.per_sample:
            return super()._do_sample_selected(op)
        colours, before = self._colours(op.args["n"])
        out = pm.PostModel._do_sample_selected(self, op)
        if self.st.tracking:
            out.update(self._tracked(colours, before, self.mask, True))
        out.update(self._deal(colours, before, self.mask))
        return out

    # ------------------------------------------------------------ the calls of the halves
    def _do_half_update(self, op):
        return {"half_buffer": self._halves().update(self.o.image_buffer).copy()}

    def _do_set_half_mode(self, op):
        if mode_of(op)[0] and not self.st.per_sample:
            return self._do_half_update(op)
        return {} if self.halves is None else {"half_buffer": self.halves.a.copy()}

    def _do_refresh(self, op):
        if self.halves is not None:
            self.halves.refresh()
        return super()._do_refresh(op)

    def _do_write_image(self, op):
        if self.halves is not None:
            self.halves.restart(self.o.image_buffer)
        return super()._do_write_image(op)

    def _do_denoise_error(self, op):
        a = op.args
        err, st, _ = hl.denoise_error(self.st.cfg, self.o.image_buffer, self.halves.a, self._features(), radius=a["radius"],
                                      threshold=a["threshold"], **a["params"])
        self.error = err
        self.events.append(("denoise_error", st[0], err.size))
        return {"denoised_error": err, "stats": (st[0], st[1], int(np.float32(st[2]).view(np.uint32)))}

    def _do_select_error(self, op):
        a = op.args
        self.mask = hl.select(self.o.image_buffer, self.halves.a, self.error, a["threshold"], a["dilate"], self.st.estimator[2])
        return {"selection": self.mask, "n_selected": int(self.mask.sum())}

    # ------------------------------------------------------------ the reprojections
    def _warp(self, op, scene_call):
        """None: no halves; False: A is zeroed; else half_mode_ref_lib.gather's (image_buffer, motion, A), from the state before the call"""
        if self.halves is None:
            return None
        a, st = op.args, self.st
        if not st.warp:
            return False
        old = cs.camera(*st.cam)
        if scene_call:
            old_sc, new_sc = self._scene(), st.table(op)
            new = None if a["cam"] is None else cs.camera(*a["cam"])
        else:
            old_sc = new_sc = self._scene()
            new = cs.camera(a["name"], a["offset"], a["vfov"])
        f0, f1 = self._features(old, old_sc), self._features(new if new is not None else old, new_sc)
        return hm.gather(st.cfg, old_sc, new_sc, old, new, self.o.image_buffer, self.halves.a, f0, f1, **a["params"])

    def _warped(self, w, out):
        if w is None:
            return out
        ib = out["image_buffer"]
        if w is False:
            self.halves.restart(ib)
        else:
            assert np.array_equal(ck.bits(w[0]), ck.bits(ib)) and np.array_equal(ck.bits(w[1]), ck.bits(out["motion"])), \
                "the gather of half A and the model's own gather disagree on the image"
            self.halves.a[:], self.halves.snapshot[:] = w[2], ib
            both = (w[2][..., 3] > 0) & (ib[..., 3] - w[2][..., 3] > 0)
            self.events.append(("warped_halves", bool(both.any()), bool((w[2][..., 3] > 0).any())))
        out["half_buffer"] = self.halves.a.copy()
        return out

    def _do_reproject(self, op):
        w = self._warp(op, False)
        return self._warped(w, super()._do_reproject(op))

    def _do_reproject_scene(self, op):
        w = self._warp(op, True)
        return self._warped(w, super()._do_reproject_scene(op))
