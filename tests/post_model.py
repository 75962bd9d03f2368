"""A CPU model of what the library keeps beside the sample path: the state behind rtpbr_reproject, rtpbr_noise_update /
rtpbr_noise_estimate / rtpbr_denoise_guided, rtpbr_set_noise_estimator, rtpbr_select_mask / rtpbr_select_noisy /
rtpbr_sample_selected and rtpbr_present, for the call sequences of tests/call_sequences.py (post_script).

``PostState`` is the plain state a context carries (configuration, scene, camera, tiles, the estimator setting, which buffers
exist, whether image_buffer still is history of this scene) and the refusal rules of include/rtpbr.h, written from the header's
"Errors" paragraphs.  The generator keeps one to stamp every operation with the code it must raise; the model keeps its own.

``PostModel`` owns an OracleRenderer and the arrays: the moments and the snapshot (noise_ref_lib.Tracker), the selection mask, the
last noise / denoised_pixels / motion / presented frame.  ``apply(op)`` returns (code, expected): the RtpbrError code the call must
raise (None: it must succeed) and {name: value} of everything the call must return or leave in a buffer.  The first-hit features
are never kept: every operation that needs them computes feature_ref_lib.features() of the model's current scene, configuration,
camera and weights, so a context that kept stale ones differs.

What the oracle has no call for is composed as the existing tests compose it: a selected launch is a full-frame sample() whose
values are taken where the mask is set (the sample index advances by n either way); a reprojection is set_camera + refresh + the
warped image_buffer written back.  After a selected launch the oracle's counters are those of a full-frame launch, so until the
next sample() only ``samples == deposits == n_selected * n`` is compared.

Two reasons for a refusal at once.  Where all reasons that hold give one code the header needs no precedence.  Where a bad
argument (EINVAL) and a bad state (ESTATE) hold together the header does not say which wins, so the generator never draws
  - a bad argument of noise_estimate, denoise_guided, select_noisy, sample_selected or reproject while tiles of world > 1 are set,
  - sample_selected(-1) in the persistent-ray form, before a select call, or with sky_kind ENVMAP before set_env,
  - a reproject with a bad parameter while set_config / set_scene / set_shape_data / set_env ran since the last refresh.
rtpbr_set_noise_estimator has no state rule and rtpbr_present's bad fields are not drawn (the Python surface refuses them first).

Readings of the header this model fixes: the moments and the snapshot come into being together (zeroed) with the first
noise_update, noise_estimate, select_noisy or denoise_guided of iterations > 0, so a write of image_buffer re-takes the snapshot
from then on; a new resolution frees the noise map with the moments; denoise_guided with iterations = 0 estimates nothing."""
import numpy as np

import call_sequences as cs
import feature_ref_lib as fr
import noise_ref_lib as nr
import pool_ref_lib as pl
import present_ref_lib as pr
import reproject_ref_lib as rr
from oracle_backend import OracleRenderer
from raytracingpbr_amd import SHAPE

EINVAL, ESTATE = cs.EINVAL, cs.ESTATE
MISSING = "no such buffer: the read must raise RtpbrError -4"
NEW_KINDS = ("noise_update", "noise_estimate", "denoise_guided", "set_noise_estimator", "select_mask", "select_noisy", "sample_selected",
             "reproject", "present")
POST_BUFFERS = ("moments", "noise", "selection", "motion", "denoised_pixels", "presented")
FEATURES = ("feature_albedo", "feature_normal", "feature_depth", "feature_object")
DIRTY_BY = ("set_config", "set_scene", "set_shape_data", "set_env")
SOURCES = {"pixels": pr.SOURCE_PIXELS, "denoised": pr.SOURCE_DENOISED, "accum": pr.SOURCE_ACCUM}
FORMATS = {"rgb8": pr.FORMAT_RGB8, "rgba8": pr.FORMAT_RGBA8}


def _finite(x):
    return x == x and abs(x) != float("inf")


def bad_argument(op):
    """True when include/rtpbr.h lists one of the call's arguments under RTPBR_EINVAL"""
    a, k = op.args, op.kind
    if k in ("noise_estimate", "select_noisy") and not a["threshold"] >= 0:
        return True
    if k == "select_noisy" and not 0 <= a["dilate"] <= 3:
        return True
    if k == "sample_selected" and a["n"] < 0:
        return True
    if k == "set_noise_estimator" and a["e"] is not None:
        pb, radius, ms = a["e"]
        return not ((pb == 0 or 3 <= pb <= 64) and 1 <= radius <= 3 and 0 <= ms <= 16777216)
    if k == "denoise_guided":
        p = a["params"]
        if not 0 <= p.get("iterations", 4) <= 8 or p.get("demodulate", 0) not in (0, 1):
            return True
        return any(not (_finite(p[s]) and p[s] > 0) for s in ("sigma_color", "sigma_normal", "sigma_depth", "variance_floor") if s in p)
    if k == "reproject":
        p = a["params"]
        mh, dt, nc = p.get("max_history", 64.0), p.get("depth_tolerance", 0.2), p.get("normal_cos", -1.0)
        return not (_finite(mh) and mh > 0 and _finite(dt) and dt >= 0 and -1 <= nc <= 1)
    return False


class PostState(cs.Mirror):
    """the context's plain state after the operations noted so far"""

    def __init__(self, base, scene0):
        super().__init__(base, scene0)
        self.cam = (scene0, (0.0, 0.0, 0.0), 1.0)
        self.estimator = (0, 3, 0)
        self.exists = set()                         # of POST_BUFFERS
        self.selected = False                       # a select call has run at this resolution
        self.dirty = {"set_config", "set_scene"}    # who ran since the last refresh / reproject (a new context: its constructor)
        self.denoised_by = None

    def state_reasons(self, op):
        """the reasons of include/rtpbr.h for RTPBR_ESTATE that hold for this call now"""
        k, why = op.kind, []
        tiled = self.tiles[3] > 1
        if k in ("features", "denoise", "noise_update", "noise_estimate", "denoise_guided", "select_mask", "select_noisy", "sample_selected",
                 "reproject") and tiled:
            why.append("tiles")
        if k == "sample_selected":
            if self.cfg.kernel_form != 0:
                why.append("persistent")
            if not self.selected:
                why.append("no_selection")
            if self.cfg.sky_kind == 1 and not self.env:
                why.append("no_env")
        if k == "reproject":
            why += [f"dirty:{d}" for d in DIRTY_BY if d in self.dirty]
        if k == "present" and op.args["source"] == "denoised" and "denoised_pixels" not in self.exists:
            why.append("no_denoised")
        return why

    def refusal(self, op):
        """(code or None, reasons) of one of the HIP-only operations.  An operation for which a bad argument and a bad state hold
        together has no code in the header: the generator must not draw it."""
        why = self.state_reasons(op)
        if bad_argument(op):
            assert not why, f"{op!r}: EINVAL and ESTATE ({why}) hold together, the header gives no precedence"
            return EINVAL, ["argument"]
        return (ESTATE, why) if why else (None, [])

    def note(self, op):
        """an operation that succeeded"""
        a, k = op.args, op.kind
        if k == "set_config":
            cfg = self.base.copy(**a["over"])
            if (cfg.width, cfg.height) != (self.cfg.width, self.cfg.height):
                self.exists.clear()
                self.selected, self.denoised_by = False, None
            self.cfg = cfg
            self.dirty.add(k)
        elif k == "set_scene":
            self.scene = a["name"]
            self.dirty.add(k)
        elif k == "set_camera":
            self.cam = (a["name"], a["offset"], 1.0)
        elif k == "set_shape_data":
            self.weights = a["variant"]
            self.dirty.add(k)
        elif k == "set_env":
            self.env = True
            self.dirty.add(k)
        elif k == "set_tiles":
            self.tiles = a["tiles"]
        elif k == "refresh":
            self.dirty.clear()
        elif k == "denoise":
            self.exists.add("denoised_pixels")
            self.denoised_by = "denoise"
        elif k == "noise_update":
            self.exists.add("moments")
        elif k == "noise_estimate":
            self.exists |= {"moments", "noise"}
        elif k == "denoise_guided":
            self.exists.add("denoised_pixels")
            self.denoised_by = "guided"
            if a["params"].get("iterations", 4) > 0:
                self.exists |= {"moments", "noise"}
        elif k == "set_noise_estimator":
            self.estimator = (0, 3, 0) if a["e"] is None else tuple(a["e"])
        elif k == "select_mask":
            self.exists.add("selection")
            self.selected = True
        elif k == "select_noisy":
            self.exists |= {"moments", "noise", "selection"}
            self.selected = True
        elif k == "reproject":
            self.cam = (a["name"], a["offset"], a["vfov"])
            self.exists.add("motion")
            self.dirty.clear()
        elif k == "present":
            self.exists.add("presented")


class PostModel:
    def __init__(self, s, threads=0):
        self.s, self.threads = s, threads
        self.o = cs.new_renderer(s, OracleRenderer, threads=threads)
        self.st = PostState(s.base, s.scene0)
        self.tracker = None                  # moments + snapshot, once they exist
        self.mask = None                     # the selection, once one exists
        self.last = {}                       # noise, denoised_pixels, motion, presented
        self.selected_work = None            # n_selected * n of the last selected launch while no sample() has run since
        self.events = []                     # what happened, for the coverage conditions of tests/test_oracle_call_sequences.py

    def close(self):
        self.o.close()

    # ------------------------------------------------------------ pieces
    def _size(self):
        return self.st.cfg.width, self.st.cfg.height

    def _features(self, cam=None):
        st = self.st
        sc = cs.scene(st.scene)
        w = cs.weights(st.weights) if any(o.type == SHAPE.BUNNY for o in sc.objects) else None
        return fr.features(sc, st.cfg, cam if cam is not None else cs.camera(*st.cam), w)

    @staticmethod
    def _named(f):
        return dict(zip(FEATURES, (f["albedo"], f["normal"], f["depth"], f["object"])))

    def _counters(self):
        c = self.o.counters()
        if self.selected_work is not None:
            return {"counters.samples_deposits": (self.selected_work, self.selected_work)}
        return {"counters": tuple(getattr(c, k) for k in cs.COUNTERS)}

    def _moments(self):
        if self.tracker is None:
            self.tracker = nr.Tracker(*self._size())
        return self.tracker.moments

    def _estimate(self, threshold):
        """the shared estimate pass: (noise, var0, stats, features); makes the moments, writes the noise map"""
        f = self._features()
        ib = self.o.image_buffer
        pb, radius, _ = self.st.estimator
        M = self._moments()
        noise, var0, stats = pl.estimate(ib, M, f["object"], threshold, pb, radius)
        if pb and (noise.view(np.uint32) != pl.estimate(ib, M, f["object"], threshold, 0, radius)[0].view(np.uint32)).any():
            self.events.append(("pooling_changed_noise",))
        self.last["noise"] = noise
        return noise, var0, stats, f, ib

    # ------------------------------------------------------------ one operation
    def apply(self, op):
        k = op.kind
        if k in ("observe", "option"):
            return None, (self._observe(op.args["what"]) if k == "observe" else {})
        if k in NEW_KINDS or k in ("features", "denoise"):
            code = self.st.refusal(op)[0]
        else:
            res = cs._apply(op, self.o)
            code = None if res is None else res[1]
        if code is not None:
            return code, {}
        size = self._size()
        had = (self.tracker is not None, self.mask is not None, "presented" in self.last)
        out = getattr(self, "_do_" + k, lambda op: {})(op)
        self.st.note(op)
        if self._size() != size:                   # a new resolution: everything beside the five sample-path buffers is gone
            if all(had):
                self.events.append(("new_resolution_with_moments_selection_presented",))
            self.tracker, self.mask, self.last = None, None, {}
        return None, out

    def _observe(self, what):
        if what == "post":
            want = {b: self.last.get(b, MISSING) for b in POST_BUFFERS}
            want["moments"] = MISSING if self.tracker is None else self.tracker.moments.copy()
            want["selection"] = MISSING if self.mask is None else self.mask
            return want
        if what == "image":
            return {"image_buffer": self.o.image_buffer}
        out = {b: getattr(self.o, b) for b in cs.BUFFERS}
        out.update(self._counters())
        return out

    # the operations the oracle has: what the model keeps beside it
    def _do_sample(self, op):
        self.selected_work = None
        return {}

    def _do_post_process(self, op):
        return {b: getattr(self.o, b) for b in ("image_pixels", "diff_buffer", "diff_pixels")}

    def _do_refresh(self, op):
        if self.tracker is not None:
            self.tracker.refresh()
        return {}

    def _do_write_image(self, op):
        if self.tracker is not None:
            self.tracker.written(self.o.image_buffer)
        return {}

    def _do_features(self, op):
        return self._named(self._features())

    def _do_denoise(self, op):
        f = self._features()
        self.last["denoised_pixels"] = fr.denoise(self.st.cfg, self.o.image_buffer, f, **op.args["params"])
        return dict(self._named(f), denoised_pixels=self.last["denoised_pixels"])

    # the operations it has not
    def _do_noise_update(self, op):
        self._moments()
        return {"moments": self.tracker.update(self.o.image_buffer).copy()}

    def _do_noise_estimate(self, op):
        noise, _, stats, _, _ = self._estimate(op.args["threshold"])
        return {"noise": noise, "stats": (stats[0], stats[1], int(np.float32(stats[2]).view(np.uint32)))}

    def _do_denoise_guided(self, op):
        p = op.args["params"]
        out = {}
        if p.get("iterations", 4) > 0:
            noise, var0, _, f, ib = self._estimate(0.0)
            out["noise"] = noise
        else:
            f, ib = self._features(), self.o.image_buffer
            var0 = np.zeros(self._size(), np.float32)
        self.last["denoised_pixels"] = nr.guided(self.st.cfg, ib, f, var0, **p)
        out["denoised_pixels"] = self.last["denoised_pixels"]
        return out

    def _do_select_mask(self, op):
        self.mask = cs.mask(*self._size(), op.args["seed"], op.args["share"])
        return {"selection": self.mask, "n_selected": int(self.mask.sum())}

    def _do_select_noisy(self, op):
        thr = op.args["threshold"]
        noise, _, _, _, ib = self._estimate(thr)
        self.mask = pl.select(noise, ib[..., 3], thr, op.args["dilate"], self.st.estimator[2])
        n, (w, h) = int(self.mask.sum()), self._size()
        self.events.append(("select_noisy", n, w * h))
        return {"noise": noise, "selection": self.mask, "n_selected": n}

    def _do_sample_selected(self, op):
        n = op.args["n"]
        before = self.o.image_buffer
        self.o.sample(n)                      # the full frame at the same sample index, which advances by n
        ib = np.where((self.mask != 0)[..., None], self.o.image_buffer, before)
        self.o.image_buffer = ib
        n_sel = int(self.mask.sum())
        self.selected_work = n_sel * n
        self.events.append(("sample_selected", n_sel, self.mask.size, n))
        return dict({"image_buffer": ib}, **self._counters())

    def _do_reproject(self, op):
        a, st = op.args, self.st
        old, new = cs.camera(*st.cam), cs.camera(a["name"], a["offset"], a["vfov"])
        f0, f1 = self._features(old), self._features(new)
        ib = self.o.image_buffer
        want_ib, motion = rr.reproject(st.cfg, old, new, ib, f0, f1, **a["params"])
        out = self._named(f1)
        if self.tracker is not None:
            ib_m, M = nr.reproject(st.cfg, old, new, ib, self.tracker.moments, f0, f1, **a["params"])
            assert np.array_equal(ib_m.view(np.uint32), want_ib.view(np.uint32)), "the two restatements of the gather disagree"
            self.tracker.moments[:], self.tracker.snapshot[:] = M, want_ib
            out["moments"] = M
        uncapped, _ = rr.reproject(st.cfg, old, new, ib, f0, f1, **dict(a["params"], max_history=3e38))
        kept = ~((motion[..., 0] == -1) & (motion[..., 1] == -1))
        self.events.append(("reproject", bool(kept.any()), bool((~kept).any()),
                            bool((uncapped[..., 3] > np.float32(a["params"].get("max_history", 64.0))).any()), self.tracker is not None))
        self.o.set_camera(new)
        self.o.refresh()
        self.o.image_buffer = want_ib
        self.last["motion"] = motion
        out.update(image_buffer=want_ib, motion=motion, ray_buffer=self.o.ray_buffer, diff_buffer=self.o.diff_buffer,
                   diff_pixels=self.o.diff_pixels)
        out.update(self._counters())
        return out

    def _do_present(self, op):
        a = op.args
        if a["source"] == "pixels":
            field = self.o.image_pixels
        elif a["source"] == "denoised":
            field = self.last["denoised_pixels"]
            if self.st.denoised_by == "guided":
                self.events.append(("present_denoised_after_guided",))
        else:       # what post_process WOULD write, from an oracle of its own that nothing else looks at
            scratch = OracleRenderer(cs.scene(self.st.scene), self.st.cfg, threads=self.threads)
            scratch.image_buffer = self.o.image_buffer
            scratch.post_process()
            field = scratch.image_pixels
            scratch.close()
        self.last["presented"] = pr.present(field, FORMATS[a["format"]], a["dither"])
        return {"presented": self.last["presented"]}
