"""One CPU model of a whole-frame context: FrameModel mirrors api.Renderer call for call and says, for every call, what the device
has to answer.

What it computes with is only what the tests already trust: the oracle's kernels for the reference's frame, tests/light_sampling_ref.py
and tests/light_grid_ref.py for the candidates, tests/temporal_reproject_ref.py, tests/temporal_motion_ref.py and
tests/temporal_unbiased_ref.py for the merge, tests/restir_unbiased_ref.py for the passes and tests/light_follow_ref.py's rebase inside
update_scene. The host rules are stated here in plain Python from the contract text of include/restir_rt_internal.h and DESIGN.md
sections 13, 14, 17 and 20-22; nothing of csrc/history_provenance.h or csrc/stage0_forms.h is compiled into it (they are code under test):

  tags      every logical reservoir buffer (RT_RES_0, RT_RES_1, RT_RES_TEMPORAL) carries the RayGenerator, the geometry generation and
            the eye it was last written under: set by generate_candidate, temporal_resampling, stage 0 and the passes of a frame, copied
            by save_temporal_reservoir, cleared by set_scene. The model keeps beside them what the device keeps in the records: the
            shaded bits of the G-buffer the buffer was made from (here: the Visibility buffer), and light_gen, the generation up to which
            the light side of the records is current.
  range     update_scene counts a generation. While rt_temporal_motion is on the vertices of one earlier generation are kept; an update
            brings them to the generation it ends if a reservoir buffer was written since the last update, and grows the range otherwise.
  merge     a temporal merge whose history carries exactly the kept generation, and that is not the current one, is a motion launch;
            otherwise one whose history's 36 camera bytes differ is a reprojecting launch, an unbiased one while rt_temporal_unbiased is
            on; otherwise it is the reference's own-pixel merge. All only while rt_temporal_reprojection is on.
  re-base   update_scene with rt_temporal_light_motion on and an emissive triangle in the old span re-bases every buffer whose light
            side is current; a span without one leaves a current buffer current.
  look-ahead  the next frame's stage 0 runs beside a frame (rt_tuning 14); every toggle, option, camera and scene call drops it. The
            model never takes it (results do not depend on it); it keeps the buffer it writes, because an update re-bases that one too,
            and it says which frames trace primary rays (rt_primary_launches).

rt_gbuffer_reuse, rt_occluder_hints, rt_neighbour_pick and every rt_tuning key change no result: the model keeps them for the predicted
form and the primary-ray count only.

Every mirrored call returns a Call: code (0, or the RT_ERR_* of a refused call, which changes nothing), error (the rt_last_error text of
a refusal), launches (the predicted instantiations, named as `c++filt` names them in the library, and "k_temporal_unbiased" where it
follows), one_launch (rt_stage0_one_launch) and out (the logical buffer a frame's resolve read)."""
import numpy as np

import light_follow_ref as lf
import light_grid_ref as lg
import restir_unbiased_ref as ru
import temporal_motion_ref as tm
import temporal_reproject_ref as tr
import temporal_unbiased_ref as tu

RT_OK, RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 0, 1, 3, 5  # include/restir_rt.h
RES_0, RES_1, RES_TEMPORAL = 0, 1, 2
FOVY = np.float32(0.9)
NAMES = ("r0", "r1", "temporal")

E_MOTION_UNBIASED = "rt_temporal_motion: rt_temporal_unbiased is on, and its ray from the history's origin would start in geometry that no longer exists"
E_UNBIASED_MOTION = "rt_temporal_unbiased: rt_temporal_motion is on, and the ray from the history's origin would start in geometry that no longer exists"
E_UNBIASED_SHADOWED = "rt_temporal_unbiased: the shadowed target function is not built for the 1/Z merge"
E_SPATIAL_SHADOWED = "rt_spatial_unbiased: the shadowed target function is not built for the 1/Z pass"
E_SPATIAL_COUNT = "rt_spatial_unbiased: %d neighbours per pass, the 1/Z pass takes at most 5"
E_EXP_GRID = "rt_light_grid: the [exp] stage-0 variants (rt_tuning keys 11 and 12) are not built for the light grid"
E_EXP_REPROJECT = "rt_temporal_reprojection / rt_temporal_motion: the [exp] stage-0 variants (rt_tuning keys 11 and 12) gather their history from the own pixel only"


def _b(v):
    return "true" if v else "false"


def gen_name(fuse, shadowed, defer, pipe, ws, raycast, power, reproject, motion, grid):
    return "k_generate_candidate<" + ", ".join(_b(v) for v in (fuse, shadowed, defer, pipe, ws, raycast, power, reproject, motion, grid)) + ">"


def temporal_name(shadowed, reproject, motion):
    return "k_temporal<" + ", ".join(_b(v) for v in (shadowed, reproject, motion)) + ">"


class Call(dict):
    __getattr__ = dict.__getitem__


def _ok(**kw):
    return Call(dict(dict(code=RT_OK, error=None, launches=(), one_launch=None, out=None), **kw))


def _refused(code, text):
    return Call(code=code, error=text, launches=(), one_launch=None, out=None)


class Tag:
    """what a buffer was written under; `shaded`: the shaded bits its records carry (the G-buffer it was made from)"""

    def __init__(self, rg, gen, eye, view):
        self.rg, self.gen, self.eye, self.view, self.light_gen = rg.copy(), gen, np.array(eye, np.float32), view, gen

    def light_current(self, geo_gen):
        return max(self.gen, self.light_gen) == geo_gen

    def key(self):
        return (self.rg.tobytes(), self.gen, self.eye.tobytes())


class Scenes:
    """one oracle scene per triangle array, one Visibility buffer per scene and camera, one grid per scene and setting"""

    def __init__(self, oracle):
        oracle.set_math_mode(oracle.MATH_PORTABLE)
        self.o, self._s, self._v, self._g = oracle, {}, {}, {}

    def scene(self, tris):
        k = tris.tobytes()
        if k not in self._s:
            self._s[k] = self.o.Scene(tris.copy(), use_bvh=True)
        return self._s[k]

    def view(self, tris, W, H, eye, at):
        k = (tris.tobytes(), W, H, np.asarray(eye, np.float32).tobytes(), np.asarray(at, np.float32).tobytes())
        if k not in self._v:
            self._v[k] = View(self.o, tris, self.scene(tris), W, H, eye, at)
        return self._v[k]

    def grid(self, tris, cells, clusters):
        k = (tris.tobytes(), cells, clusters)
        if k not in self._g:
            self._g[k] = lg.Grid(tris.copy(), cells, clusters)
        return self._g[k]


class View:
    def __init__(self, oracle, tris, scene, W, H, eye, at):
        self.W, self.H, self.eye, self.at = W, H, np.asarray(eye, np.float32), np.asarray(at, np.float32)
        self.rg = oracle.raygen_lookat(self.eye, self.at, (0, 1, 0), FOVY, W, H)
        self.vis = scene.raycast(W, H, self.rg)
        hit = self.vis["index"] >= 0
        self.shaded = hit & ~(tris["emissive"] > 0).any(axis=1)[np.maximum(self.vis["index"], 0)]


class FrameModel:
    def __init__(self, oracle, W, H, scenes=None, exp=False):
        self.o, self.W, self.H, self.exp = oracle, W, H, exp
        self.sc = scenes or Scenes(oracle)
        self.tris = None
        self.eye = self.at = self.view = None
        self.opt = oracle.default_options()
        st = oracle.new_state(W, H)
        self.buf = dict(r0=st["r0"], r1=st["r1"], temporal=st["temporal"])
        self.accum, self.pixels = st["accum"], st["pixels"]
        self.tag = dict(r0=None, r1=None, temporal=None)
        # the switches
        self.reproject = self.motion = self.t_unbiased = self.s_unbiased = self.light_follow = False
        self.power, self.grid = False, None
        self.gbuffer_reuse_on, self.hints_on, self.pick_mode = True, True, 1
        self.tune = {11: 0, 12: 0, 13: 1, 14: -1, 16: -1, 17: -1, 20: 1, 25: -1}
        self.walk_on = False
        # the moved range
        self.geo_gen = self.kept_gen = 0
        self.lo = self.hi = 0
        self.kept, self.dirty = None, False  # the triangles of generation kept_gen while rt_temporal_motion is on
        # state that other calls invalidate
        self.epoch = 0
        self.gbuf_valid, self.traced_epoch, self.gview = False, -1, None
        self.ahead = None  # dict(epoch, reuse) of a look-ahead that is still good
        self.spare, self.spare_tag = None, None  # the buffer the look-ahead's candidates went to
        self.primary_launches = 0
        self.last_rebased = 0
        self.reset_stats()
        self.lf_stats = dict(buffers=0, examined=0, located=0, moved=0, emptied=0)
        # what the conditions of tests/test_frame_model_cpu.py ask of a case
        self.seen = dict(reuse_frames=0, reprojected_from_another_pixel=0, motion_valid=0, motion_elsewhere=0, records_moved=0, kept_out_of_z=0,
                         unbiased_launches=0, motion_launches=0, refused=0, grid_frames_after_a_light_move=0)
        self._light_moved = False

    def reset_stats(self):
        self.reproject_stats = dict(merged=0, valid=0, moved=0)
        self.motion_stats = dict(merged=0, in_range=0, valid=0)
        self.unbiased_stats = dict(merged=0, valid=0, excluded=0, history_rays=0)

    # ------------------------------------------------------------------------------------------------------ scene and camera
    def _changed(self):
        self.epoch += 1
        self.ahead = None

    def set_scene(self, tris):
        self.tris = np.ascontiguousarray(tris).copy()
        self.tag = dict(r0=None, r1=None, temporal=None)
        self.spare_tag = None
        self.geo_gen = self.kept_gen = 0
        self.lo = self.hi = 0
        self.dirty = False
        self.kept = self.tris.copy() if self.motion else None
        self.gbuf_valid = False
        self._changed()
        self._look()
        return _ok()

    def lookat(self, eye, at):
        self.eye, self.at = np.asarray(eye, np.float32), np.asarray(at, np.float32)
        self._changed()
        self._look()
        return _ok()

    def _look(self):
        self.view = self.sc.view(self.tris, self.W, self.H, self.eye, self.at) if self.tris is not None and self.eye is not None else None

    def set_options(self, opt):
        self.opt = np.array(opt, copy=True)
        self._changed()
        return _ok()

    def walk_stats_enable(self, on):
        self.walk_on = bool(on)
        self.reset_stats()
        return _ok()

    def _buffers(self):
        out = [(n, self.buf[n], self.tag[n]) for n in NAMES if self.tag[n] is not None]
        if self.spare_tag is not None:
            out.append(("spare", self.spare, self.spare_tag))
        return out

    def update_scene(self, span, first):
        span = np.ascontiguousarray(span)
        n = len(span)
        old, new = self.tris, self.tris.copy()
        new[first:first + n] = span
        self.last_rebased = 0
        if self.light_follow:
            if not (old["emissive"][first:first + n] > 0).any():
                for _, _, t in self._buffers():
                    if t.light_current(self.geo_gen):
                        t.light_gen = self.geo_gen + 1
            else:
                for _, b, t in self._buffers():
                    if not t.light_current(self.geo_gen):
                        continue
                    sh = t.view.shaded
                    m = b.copy()
                    m["M"][~sh] = 0  # the kernel examines the records with the shaded bit and M > 0
                    out, _, _, counts = lf.rebase(m, old, new, first, n)
                    b[sh] = out[sh]
                    t.light_gen = self.geo_gen + 1
                    self.last_rebased += 1
                    for k, v in counts.items():
                        self.lf_stats[k] += v
                    self.seen["records_moved"] += counts["moved"]
                self.lf_stats["buffers"] += self.last_rebased
                self._light_moved = True
        # the moved range
        if self.kept is not None:
            if self.motion and self.dirty:
                self.kept, self.kept_gen, self.lo, self.hi = old.copy(), self.geo_gen, first, first + n
            elif self.hi > self.lo:
                self.lo, self.hi = min(self.lo, first), max(self.hi, first + n)
            else:
                self.lo, self.hi = first, first + n
        self.geo_gen += 1
        self.dirty = False
        self.tris = new
        self._changed()
        self._look()
        return _ok()

    # ------------------------------------------------------------------------------------------------------------- switches
    def gbuffer_reuse(self, on):
        self.gbuffer_reuse_on = bool(on)
        self.ahead = None
        return _ok()

    def occluder_hints(self, on):
        self.hints_on = bool(on)
        self.ahead = None
        return _ok()

    def neighbour_pick(self, mode):
        self.pick_mode = int(mode)
        return _ok()

    def tuning(self, key, value):
        self.tune[key] = value
        if key == 14 and value == 0:
            self.ahead = None
        if key == 14 and value == 1:
            self._outside()
        return _ok()

    def spatial_unbiased(self, on):
        self.s_unbiased = bool(on)
        self.epoch += 1  # the contract: changes rt_state_epoch, as rt_options_set does (which is what stales the look-ahead)
        self.ahead = None
        return _ok()

    def light_sampling(self, mode):
        self.power = mode in ("power", 1)
        self._changed()
        return _ok()

    def light_grid(self, cells, clusters=64):
        self.grid = (int(cells), int(clusters)) if cells else None
        self._changed()
        return _ok()

    def temporal_reprojection(self, on):
        self.reproject = bool(on)
        self._changed()
        return _ok()

    def temporal_motion(self, on):
        if on and self.t_unbiased:
            self.seen["refused"] += 1
            return _refused(RT_ERR_UNSUPPORTED, E_MOTION_UNBIASED)
        self._changed()
        if bool(on) != self.motion:
            # going on the current vertices are kept (updates before it are not followed), going off they are freed
            self.motion = bool(on)
            self.kept_gen, self.lo, self.hi = self.geo_gen, 0, 0
            self.kept = self.tris.copy() if self.motion and self.tris is not None else None
        return _ok()

    def temporal_unbiased(self, on):
        if on and self.motion:
            self.seen["refused"] += 1
            return _refused(RT_ERR_UNSUPPORTED, E_UNBIASED_MOTION)
        self.t_unbiased = bool(on)
        self._changed()
        return _ok()

    def temporal_light_motion(self, on):
        if on and not self.light_follow:
            self.lf_stats = dict(buffers=0, examined=0, located=0, moved=0, emptied=0)
        self.light_follow = bool(on)
        self._changed()
        return _ok()

    def motion_range(self):
        return dict(lo=self.lo, hi=self.hi, generation=self.kept_gen)

    # ---------------------------------------------------------------------------------------------------------------- forms
    def _opt(self, k):
        return int(self.opt[k][0])

    def _selection(self):
        ris = self._opt("ris_sample_count") > 0
        grid = self.grid is not None and ris
        return grid, (not grid and self.power and ris)

    def _history_kind(self, tag):
        """'motion', 'camera' or 'own': what a merge that reads a buffer under `tag` is"""
        if not self.reproject or not self._opt("use_temporal_resampling") or tag is None:
            return "own"
        if self.motion and self.kept is not None and tag.gen == self.kept_gen and self.kept_gen != self.geo_gen:
            return "motion"
        return "camera" if tag.rg.tobytes() != self.view.rg.tobytes() else "own"

    def _exp_form(self):
        return self.exp and not self._opt("use_shadowed_target_function") and (self.tune[11] or self.tune[12])

    def _one_launch_wanted(self):
        """the whole frame's stage 0 in one launch: rt_tuning 25, the product's fused unshadowed kernel with the work-sharing walk,
        primary rays not through it (rt_tuning 16 = 0: at these sizes 'auto' is a launch of one generation of wavefronts)"""
        return (self.tune[25] != 0 and not (self.exp and (self.tune[11] or self.tune[12])) and self._opt("use_temporal_resampling")
                and not self._opt("use_shadowed_target_function") and self.tune[13] == 1 and self.tune[16] == 0)

    def _stage0(self, fuse, hist, raycast):
        """the candidates' launch: a refusal, or (kind of history, launches)"""
        sh = bool(self._opt("use_shadowed_target_function"))
        grid, power = self._selection()
        kind = self._history_kind(hist) if fuse else "own"
        ub = kind == "camera" and self.t_unbiased
        if ub and sh:
            return _refused(RT_ERR_UNSUPPORTED, E_UNBIASED_SHADOWED), None
        defer = pipe = False
        if self.exp and fuse and not sh and (self.tune[11] or self.tune[12]):
            if grid:
                return _refused(RT_ERR_UNSUPPORTED, E_EXP_GRID), None
            if kind != "own":
                return _refused(RT_ERR_UNSUPPORTED, E_EXP_REPROJECT), None
            defer, pipe = bool(self.tune[11]), bool(self.tune[12])
        ws = fuse and not sh and not defer and not pipe and self.tune[13] == 1
        name = gen_name(fuse, sh, defer, pipe, ws, ws and raycast, power, kind != "own", kind == "motion", grid)
        return None, ("unbiased" if ub else kind, (name,) + (("k_temporal_unbiased",) if ub else ()))

    # ------------------------------------------------------------------------------------------------------------ the kernels
    def _write_tag(self, name, view=None):
        self.tag[name] = Tag(self.view.rg, self.geo_gen, self.view.eye, view or self.view)
        self.dirty = True

    def _candidates(self, frame, res):
        v = self.view
        grid, power = self._selection()
        if grid:
            return lg.generate_candidate(self.W, self.H, frame, self.tris, v.vis, v.eye, self.opt, lg.GRID, res, grid=self.sc.grid(self.tris, *self.grid))
        return lg.generate_candidate(self.W, self.H, frame, self.tris, v.vis, v.eye, self.opt, lg.POWER if power else lg.UNIFORM, res)

    def _merge(self, frame, kind, hist, tag, res, count=True):
        """the history `hist` (written under `tag`) merged into `res` in place"""
        W, H, v, opt = self.W, self.H, self.view, self.opt
        q = np.arange(W * H)
        if kind == "own":
            self.sc.scene(self.tris).temporal_resampling(W, H, frame, v.vis, v.eye, opt, hist, res)
            return
        pv = tag.view
        same = tag.rg.tobytes() == v.rg.tobytes()
        if kind == "motion":
            _, d = tm.temporal(W, H, frame, self.tris, self.kept, v.vis, pv.vis, v.eye, tag.eye, tag.rg, v.rg, self.lo, self.hi, opt, hist, res)
            inr, valid = d[:, 3] == 1, d[:, 0] == 1
            other = valid & ((d[:, 1] != q % W) | (d[:, 2] != q // W))
            self.seen["motion_launches"] += 1
            self.seen["motion_valid"] += int((inr & valid).sum())
            self.seen["motion_elsewhere"] += int((inr & other).sum())
            if count and self.walk_on:
                for k, n in (("merged", v.shaded.sum()), ("in_range", inr.sum()), ("valid", (inr & valid).sum())):
                    self.motion_stats[k] += int(n)
                if not same:  # the pixels off the range take the reprojection's path
                    out = v.shaded & ~inr
                    for k, n in (("merged", out.sum()), ("valid", (out & valid).sum()), ("moved", (out & other).sum())):
                        self.reproject_stats[k] += int(n)
            return
        if kind == "camera":
            _, d = tr.temporal(W, H, frame, self.tris, v.vis, pv.vis, v.eye, tag.rg, v.rg, opt, hist, res)
            valid = d[:, 0] == 1
            other = valid & ((d[:, 1] != q % W) | (d[:, 2] != q // W))
        else:
            _, d = tu.temporal(W, H, frame, self.tris, v.vis, pv.vis, v.eye, tag.rg, v.rg, opt, hist, res)
            valid = d[:, 0] == 1
            pts, _ = tr.surface_points(self.tris, v.vis, v.eye)
            pix, _ = tr.project(pts, tag.rg, W, H)
            other = valid & ((pix[:, 1] != q % W) | (pix[:, 2] != q // W))
            ex = (d[:, 4] > 0) & (d[:, 2] == 0)
            self.seen["unbiased_launches"] += 1
            self.seen["kept_out_of_z"] += int(ex.sum())
            if count and self.walk_on:
                for k, n in (("merged", v.shaded.sum()), ("valid", (d[:, 4] > 0).sum()), ("excluded", ex.sum()), ("history_rays", d[:, 3].sum())):
                    self.unbiased_stats[k] += int(n)
        self.seen["reprojected_from_another_pixel"] += int(other.sum())
        if count and self.walk_on:
            for k, n in (("merged", v.shaded.sum()), ("valid", valid.sum()), ("moved", other.sum())):
                self.reproject_stats[k] += int(n)

    def _spatial_check(self):
        if not (self.s_unbiased and self._opt("use_spatial_resampling")):
            return None
        if self._opt("use_shadowed_target_function"):
            return _refused(RT_ERR_UNSUPPORTED, E_SPATIAL_SHADOWED)
        if self._opt("spatial_resampling_sample_count") > 5:
            return _refused(RT_ERR_UNSUPPORTED, E_SPATIAL_COUNT % self._opt("spatial_resampling_sample_count"))
        return None

    def _pass(self, frame, k, src, dst):
        v = self.view
        if self.s_unbiased and self._opt("use_spatial_resampling"):
            self.buf[dst] = ru.spatial(self.W, self.H, frame, k, self.tris, v.vis, v.eye, self.opt, self.buf[src])[0]
        else:
            self.buf[dst] = self.sc.scene(self.tris).spatial_resampling(self.W, self.H, frame, k, v.vis, v.eye, self.opt, self.buf[src])
        self._write_tag(dst)

    def _traced(self):
        self.primary_launches += 1
        self.gbuf_valid, self.traced_epoch, self.gview = True, self.epoch, self.view

    def _outside(self):
        """a reservoir buffer changed outside the staged frame: the look-ahead's candidates are stale, its primary rays are not"""
        if self.ahead is not None:
            self.ahead["gen_frame"] = None

    def _reusable(self):
        return self.gbuffer_reuse_on and not self.walk_on and self.gbuf_valid and self.traced_epoch == self.epoch

    # ------------------------------------------------------------------------------------------------ the per-kernel entry points
    def raycast(self):
        self._traced()
        return _ok()

    def gbuffer_is_current(self):
        """was the G-buffer traced under the current camera and scene? (a per-kernel call reads it as it lies)"""
        return self.gbuf_valid and self.gview is self.view

    def generate_candidate(self, frame, dst=RES_0):
        refusal, plan = self._stage0(False, None, False)
        if refusal:
            return refusal
        self._candidates(frame, self.buf[NAMES[dst]])
        self._write_tag(NAMES[dst])
        self._outside()
        return _ok(launches=plan[1])

    def temporal_resampling(self, frame, prev=RES_TEMPORAL, inout=RES_0):
        if prev == inout:
            return _refused(RT_ERR_ARG, "prev and inout must differ")
        p, i = NAMES[prev], NAMES[inout]
        kind = self._history_kind(self.tag[p])
        sh = bool(self._opt("use_shadowed_target_function"))
        if kind == "camera" and self.t_unbiased:
            if sh:
                self.seen["refused"] += 1
                return _refused(RT_ERR_UNSUPPORTED, E_UNBIASED_SHADOWED)
            kind, launches = "unbiased", ("k_temporal_unbiased",)
        else:
            launches = (temporal_name(sh, kind != "own", kind == "motion"),)
        made_from = self.tag[i].view if self.tag[i] is not None else self.view  # merged in place: its shaded bits stay
        self._merge(frame, kind, self.buf[p], self.tag[p], self.buf[i])
        self._write_tag(i, made_from)
        self._outside()
        return _ok(launches=launches)

    def save_temporal_reservoir(self, src=RES_0, dst=RES_TEMPORAL):
        if src != dst:
            self.buf[NAMES[dst]][:] = self.buf[NAMES[src]]
            t = self.tag[NAMES[src]]
            self.tag[NAMES[dst]] = None if t is None else self._copy_tag(t)
        self._outside()
        return _ok()

    @staticmethod
    def _copy_tag(t):
        c = Tag(t.rg, t.gen, t.eye, t.view)
        c.light_gen = t.light_gen
        return c

    def spatial_resampling(self, frame, k, src, dst):
        refusal = self._spatial_check()
        if refusal:
            self.seen["refused"] += 1
            return refusal
        self._pass(frame, k, NAMES[src], NAMES[dst])
        return _ok()

    def resolve(self, res):
        v = self.view
        self.sc.scene(self.tris).resolve(self.accum, self.W, self.H, v.vis, v.eye, self.opt, self.buf[NAMES[res]])
        return _ok()

    def tone_mapping(self):
        self.pixels = self.o.tone_mapping(self.accum, self.W, self.H)
        return _ok()

    # ---------------------------------------------------------------------------------------------------------------- frame
    def frame(self, frame, clear_first=False):
        """rt_frame. A frame the unbiased passes refuse has done nothing. One whose stage 0 is refused has written no reservoir buffer,
        no tag and no range; its clear and its primary rays come before the candidates' launch and have happened"""
        passes = self._opt("spatial_resampling_passes")
        refusal = self._spatial_check() if passes > 0 else None
        if refusal:
            self.seen["refused"] += 1
            return refusal
        fuse = bool(self._opt("use_temporal_resampling"))
        # primary rays: taken from a look-ahead that is still good, not needed (rt_gbuffer_reuse), or traced
        take = self.ahead is not None and self.tune[14] != 0 and self.ahead["epoch"] == self.epoch and (not self.ahead["reuse"] or self._reusable())
        reuse = (take and self.ahead["reuse"]) or (not take and self._reusable())
        defer = not take and not reuse and self._one_launch_wanted()
        refusal, plan = self._stage0(fuse, self.tag["temporal"], defer)
        if clear_first:
            self.o.clear(self.accum, self.W, self.H)
        if take and not self.ahead["reuse"]:
            self.gbuf_valid, self.traced_epoch, self.gview = True, self.epoch, self.view  # the set the look-ahead traced (and counted) becomes the current one
        elif not reuse:
            self._traced()
        taken = take and self.tune[14] in (-1, 2) and self.ahead["gen_frame"] == frame  # its candidates too
        self.ahead = None
        if refusal:
            self.seen["refused"] += 1
            return refusal
        kind, launches = plan
        self.seen["reuse_frames"] += int(reuse)
        if self.grid is not None and self._light_moved:
            self.seen["grid_frames_after_a_light_move"] += 1
        self._light_moved = False
        one_launch = defer or (reuse and not taken and self._one_launch_wanted())
        # stage 0
        self._candidates(frame, self.buf["r0"])
        if fuse:
            self._merge(frame, kind, self.buf["temporal"], self.tag["temporal"], self.buf["r0"])
        self._write_tag("r0")
        self.save_temporal_reservoir(RES_0, RES_TEMPORAL)
        # the look-ahead: the next frame's stage 0 under this camera, into a buffer of its own
        self._look_ahead(frame)
        src, dst = "r0", "r1"
        for k in range(passes):
            if k:
                src, dst = dst, src
            self._pass(frame, k, src, dst)
        out = NAMES.index(dst)
        self.resolve(out)
        self.tone_mapping()
        return _ok(launches=launches, one_launch=one_launch, out=out)

    def _look_ahead(self, frame):
        if self.tune[14] == 0:
            self.ahead = None
            return
        reuse = self._reusable()
        generate = self.tune[14] in (-1, 2) and not (self.exp and self.tune[11])
        if reuse and not generate:
            self.ahead = None
            return
        if not reuse:
            self.primary_launches += 1
        if generate:
            # its candidates, merged with the history this frame has just saved (same camera, same generation: the own-pixel merge);
            # kept because an update re-bases this buffer as any other
            self.spare = self._candidates(frame + 1, np.zeros_like(self.buf["r0"]))
            if self._opt("use_temporal_resampling"):
                self._merge(frame + 1, "own", self.buf["temporal"], self.tag["temporal"], self.spare, count=False)
            self.spare_tag = Tag(self.view.rg, self.geo_gen, self.view.eye, self.view)
        self.ahead = dict(epoch=self.epoch, reuse=reuse, gen_frame=frame + 1 if generate else None)
