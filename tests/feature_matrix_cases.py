"""The cases of tests/test_gpu_feature_matrix.py and the one driver that runs a case through tests/frame_model.py alone (the conditions
and the census of tests/test_frame_model_cpu.py) or through the model and a device context side by side.

The moving world: the lamp room of tests/light_sampling_ref.py, FRAMES frames. Between two frames the box (BOX_LO:BOX_HI) moves by one
rt_scene_update, the panel (P0:P0 + 2) by a second one with no frame between them, and the camera orbits ORBIT rad. The box starts 2
units back and comes forward 1 unit per frame: what tests/test_gpu_temporal_motion.py found that 8 x 8 needs to gather from other pixels."""
import ctypes as C
from collections import namedtuple

import numpy as np

import frame_model as fm
import light_sampling_ref as ls
from cedec_2024_rt_amd import scenes as _scenes

FRAMES, ORBIT = 5, 0.1
BOX_LO, BOX_HI = 64, 76
BOX_START, BOX_STEP, PANEL_STEP = (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), (0.3, 0.0, -0.1)
BASE = ls.make_lamp_room()
P0 = int(np.where(BASE["emissive"][:, 0] == np.float32(20.0))[0][0])
GRID = (16, 64)
SHAPES = ("one launch", "two launches", "two launches, no work sharing", "shadowed")
SELECTIONS = ("uniform", "power", "grid")
HISTORIES = ("own pixel", "reproject", "motion")

Case = namedtuple("Case", "W H shape selection history follow t_unbiased s_unbiased path exp")


def case(W=37, H=29, shape="one launch", selection="uniform", history="own pixel", follow=True, t_unbiased=False, s_unbiased=False, path="frame", exp=()):
    return Case(W, H, shape, selection, history, follow, t_unbiased, s_unbiased, path, tuple(exp))


def case_id(c):
    s = f"{c.W}x{c.H}-{c.shape}-{c.selection}-{c.history}".replace(" ", "_").replace(",", "")
    return s + ("-follow" if c.follow else "") + ("-tu" if c.t_unbiased else "") + ("-su" if c.s_unbiased else "") + ("-kernels" if c.path == "kernels" else "") + "".join(f"-exp{k}" for k in c.exp)


def _cases():
    out = []
    # every fused row: 4 stage-0 shapes x 3 light selections x 3 histories, with rt_temporal_light_motion off and on
    for shape in SHAPES:
        for sel in SELECTIONS:
            for hist in HISTORIES:
                for follow in (False, True):
                    out.append(case(shape=shape, selection=sel, history=hist, follow=follow))
    # the nine {selection x history} pairs of the one-launch shape at one tile and at whole tiles
    for W, H in ((8, 8), (64, 48)):
        for sel in SELECTIONS:
            for hist in HISTORIES:
                out.append(case(W, H, selection=sel, history=hist))
    # rt_temporal_unbiased over the unshadowed reproject rows
    for shape in SHAPES[:3]:
        for sel in SELECTIONS:
            out.append(case(shape=shape, selection=sel, history="reproject", t_unbiased=True))
    # rt_spatial_unbiased over the one-launch rows
    for sel in SELECTIONS:
        for hist in HISTORIES:
            out.append(case(selection=sel, history=hist, s_unbiased=True))
    # both
    for sel in SELECTIONS:
        out.append(case(selection=sel, history="reproject", t_unbiased=True, s_unbiased=True))
    # the per-kernel path: the unfused rows, k_temporal's rows, k_temporal_unbiased through rt_temporal_resampling
    for shape in ("one launch", "shadowed"):
        for sel, hist in zip(SELECTIONS, HISTORIES):
            out.append(case(shape=shape, selection=sel, history=hist, path="kernels"))
    out.append(case(selection="power", history="reproject", t_unbiased=True, path="kernels"))
    return out


CASES = _cases()
# the experiments library's six rows: rt_tuning 11 and 12, uniform and power, a camera that stands still
EXP_CASES = [case(selection=sel, follow=False, exp=keys) for keys in ((11,), (12,), (11, 12)) for sel in ("uniform", "power")]


def move(tris, offset, first, count):
    m = np.zeros(len(tris), bool)
    m[first:first + count] = True
    return _scenes.move_triangles(tris, m, offset)


def orbit(angle):
    e, a = np.asarray(ls.LAMP_EYE, np.float32).astype(np.float64), np.asarray(ls.LAMP_AT, np.float32).astype(np.float64)
    c, s = np.cos(angle), np.sin(angle)
    d = e - a
    return np.asarray(a + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]]), np.float32), np.asarray(ls.LAMP_AT, np.float32)


def start_scene():
    return move(BASE, BOX_START, BOX_LO, BOX_HI - BOX_LO)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def eq_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def res_diff(a, b, mask):
    bad = []
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = np.ascontiguousarray(a[f][mask]), np.ascontiguousarray(b[f][mask])
        if not eq_bits(x, y):
            bad.append((f, int((bits(x).reshape(len(x), -1) != bits(y).reshape(len(y), -1)).any(axis=1).sum())))
    return bad


class Pair:
    """the model and, where there is one, a device context: every call goes to both, and the device answers what the model says"""

    def __init__(self, oracle, W, H, scenes, api=None, exp=False, log=None):
        self.m = fm.FrameModel(oracle, W, H, scenes=scenes, exp=exp)
        self.api, self.log = api, log if log is not None else []
        self.r = [api.Renderer(W, H, exp=exp)] if api else []
        self.W, self.H = W, H

    def close(self):
        for r in self.r:
            r.close()

    def _raw(self, r, name, *args):
        return getattr(r.L, name)(r.h, *args)

    def call(self, what, model_call, raw, *args, only=None):
        """model_call(): the model's Call; raw: the C entry point, called with *args on every context (or on `only`)"""
        self.log.append(what)
        want = model_call() if model_call else None
        for r in (self.r if only is None else only):
            before = self.state(r) if want is not None and want.code else None
            rc = self._raw(r, raw, *args)
            if want is None:
                assert rc == 0, f"{what}: {rc} {r.L.rt_last_error(r.h).decode()}\n{self.log}"
                continue
            assert rc == want.code, f"{what}: the device answers {rc} ({r.L.rt_last_error(r.h).decode()}), the model {want.code}\n{self.log}"
            if want.code:
                assert r.L.rt_last_error(r.h).decode() == want.error, f"{what}: {r.L.rt_last_error(r.h).decode()!r}\n{self.log}"
                after = self.state(r)
                for k in before:
                    assert eq_bits(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], f"{what}: a refused call changed {k}\n{self.log}"
        return want

    def state(self, r):
        """what a refused call must leave alone"""
        e = C.c_uint64()
        assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
        s = dict(epoch=e.value, range=r.temporal_motion_range())
        for k, b in enumerate((self.api.RT_BUF_RES_0, self.api.RT_BUF_RES_1, self.api.RT_BUF_RES_TEMPORAL)):
            s[f"buffer {k}"] = r.download(b)
            cam, sc = r.reservoir_camera(k), r.reservoir_scene(k)
            s[f"camera tag {k}"] = None if cam is None else cam.tobytes()
            s[f"scene tag {k}"] = None if sc is None else (sc[0], sc[1].tobytes())
        return s

    # the mirrored calls
    def set_scene(self, tris):
        self.log.append("set_scene")
        self.m.set_scene(tris)
        for r in self.r:
            r.set_scene(tris)

    def update_scene(self, tris, first, count, what):
        self.log.append(f"update_scene {what}")
        self.m.update_scene(tris[first:first + count], first)
        for r in self.r:
            r.update_scene(tris[first:first + count], first=first)
            got = r.temporal_light_motion()["rebased"]
            if len(self.r) == 1:  # a context with other knobs may rotate through other buffers
                assert got == self.m.last_rebased, f"{what}: {got} buffers re-based, the model says {self.m.last_rebased}\n{self.log}"

    def lookat(self, eye, at):
        self.log.append(f"lookat {np.asarray(eye).tolist()}")
        self.m.lookat(eye, at)
        for r in self.r:
            r.lookat(eye, at, fovy=fm.FOVY)
            assert eq_bits(r.raygen(), self.m.view.rg)

    def set_options(self, opt):
        self.log.append("set_options " + ", ".join(f"{k}={opt[k][0]}" for k in ("use_shadowed_target_function", "spatial_resampling_passes", "accumulate", "spatial_resampling_sample_count")))
        self.m.set_options(opt)
        for r in self.r:
            r.set_options(opt)

    def tuning(self, key, value, only=None):
        """on every context, or on those of `only` (the model follows either way: it is context A's)"""
        self.log.append(f"tuning {key} = {value}" + (" (A)" if only is not None else ""))
        self.m.tuning(key, value)
        for r in (self.r if only is None else only):
            r.tuning(key, value)

    def walk_stats_enable(self, on):
        self.m.walk_stats_enable(on)
        for r in self.r:
            r.walk_stats_enable(on)

    def light_sampling(self, mode):
        self.call(f"light_sampling {mode}", lambda: self.m.light_sampling(mode), "rt_light_sampling", 1 if mode == "power" else 0)

    def light_grid(self, cells, clusters=64):
        self.call(f"light_grid {cells} {clusters}", lambda: self.m.light_grid(cells, clusters), "rt_light_grid", cells, clusters)

    def temporal_reprojection(self, on):
        self.call(f"temporal_reprojection {on}", lambda: self.m.temporal_reprojection(on), "rt_temporal_reprojection", int(on))

    def temporal_motion(self, on):
        return self.call(f"temporal_motion {on}", lambda: self.m.temporal_motion(on), "rt_temporal_motion", int(on))

    def temporal_unbiased(self, on):
        return self.call(f"temporal_unbiased {on}", lambda: self.m.temporal_unbiased(on), "rt_temporal_unbiased", int(on))

    def spatial_unbiased(self, on):
        self.call(f"spatial_unbiased {on}", lambda: self.m.spatial_unbiased(on), "rt_spatial_unbiased", int(on))

    def temporal_light_motion(self, on):
        self.call(f"temporal_light_motion {on}", lambda: self.m.temporal_light_motion(on), "rt_temporal_light_motion", int(on))

    def frame(self, n, clear_first=False):
        """rt_frame on every context; returns the model's Call. A launched frame is checked bit for bit"""
        self.log.append(f"frame {n}" + (" clear_first" if clear_first else ""))
        want = self.m.frame(n, clear_first)
        for r in self.r:
            before = self.state(r) if want.code else None
            out = C.c_int(-1)
            rc = r.L.rt_frame(r.h, int(n), int(clear_first), C.byref(out))
            err = r.L.rt_last_error(r.h).decode()
            assert rc == want.code, f"frame {n}: the device answers {rc} ({err}), the model {want.code} ({want.error})\n{self.log}"
            if want.code:
                assert err == want.error, f"frame {n}: {err!r}\n{self.log}"
                after = self.state(r)
                for k in before:
                    assert eq_bits(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], f"frame {n}: a refused frame changed {k}\n{self.log}"
            else:
                assert out.value == want.out, f"frame {n}: resolve read buffer {out.value}, the model says {want.out}\n{self.log}"
        if not want.code:
            self.check(f"frame {n}", want.out)
        return want

    def kernels(self, n):
        """the frame kernel by kernel (Renderer.frame_by_kernels); returns the launches the model predicts"""
        self.log.append(f"frame {n} by kernels")
        launches = []
        passes = int(self.m.opt["spatial_resampling_passes"][0])
        steps = [("rt_raycast", lambda: self.m.raycast(), ()), ("rt_generate_candidate", lambda: self.m.generate_candidate(n, 0), (n, 0)),
                 ("rt_temporal_resampling", lambda: self.m.temporal_resampling(n, 2, 0), (n, 2, 0)), ("rt_save_temporal_reservoir", lambda: self.m.save_temporal_reservoir(0, 2), (0, 2))]
        src, dst = 0, 1
        for k in range(passes):
            if k:
                src, dst = dst, src
            steps.append(("rt_spatial_resampling", (lambda k=k, s=src, d=dst: self.m.spatial_resampling(n, k, s, d)), (n, k, src, dst)))
        steps += [("rt_resolve", lambda: self.m.resolve(dst), (dst,)), ("rt_tone_mapping", lambda: self.m.tone_mapping(), ())]
        for raw, mc, args in steps:
            want = mc()
            assert want.code == 0, (raw, want)
            launches += list(want.launches)
            for r in self.r:
                rc = self._raw(r, raw, *args)
                assert rc == 0, f"{raw}{args}: {rc} {r.L.rt_last_error(r.h).decode()}\n{self.log}"
        self.check(f"frame {n} by kernels", dst)
        return launches

    def check(self, what, out):
        """every context holds the model's bytes: accumulation, pixels, the last pass's records and the history on the shaded pixels, the
        tags of the three buffers and the moved range"""
        m, api = self.m, self.api
        sh = m.view.shaded
        for i, r in enumerate(self.r):
            who = f"{what} (context {'AB'[i]})"
            acc = r.download(api.RT_BUF_ACCUMULATION)
            assert eq_bits(acc, m.accum.reshape(acc.shape)), f"{who}: accumulation\n{self.log}"
            assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(self.H, self.W, 4), m.pixels), f"{who}: pixels\n{self.log}"
            bad = res_diff(r.download(api.RT_BUF_RES_0 + out), m.buf[fm.NAMES[out]], sh)
            assert not bad, f"{who}: records after the frame {bad} of {int(sh.sum())}\n{self.log}"
            bad = res_diff(r.download(api.RT_BUF_RES_TEMPORAL), m.buf["temporal"], sh)
            assert not bad, f"{who}: temporal history {bad} of {int(sh.sum())}\n{self.log}"
            for k, name in enumerate(fm.NAMES):
                t, cam, sc = m.tag[name], r.reservoir_camera(k), r.reservoir_scene(k)
                if t is None:
                    assert cam is None and sc is None, f"{who}: buffer {k} carries a tag\n{self.log}"
                else:
                    assert cam is not None and eq_bits(cam, t.rg), f"{who}: rt_reservoir_camera {k}\n{self.log}"
                    assert sc is not None and sc[0] == t.gen and eq_bits(sc[1], t.eye), f"{who}: rt_reservoir_scene {k}: {sc}, the model {t.gen} {t.eye}\n{self.log}"
            assert r.temporal_motion_range() == m.motion_range(), f"{who}: rt_temporal_motion_range {r.temporal_motion_range()}, the model {m.motion_range()}\n{self.log}"

    def check_stats(self):
        m = self.m
        for r in self.r:
            assert r.temporal_reprojection_stats() == m.reproject_stats, f"rt_temporal_reprojection_stats {r.temporal_reprojection_stats()}, the model {m.reproject_stats}"
            assert r.temporal_motion_stats() == m.motion_stats, f"rt_temporal_motion_stats {r.temporal_motion_stats()}, the model {m.motion_stats}"
            assert r.temporal_unbiased_stats() == m.unbiased_stats, f"rt_temporal_unbiased_stats {r.temporal_unbiased_stats()}, the model {m.unbiased_stats}"
            if m.light_follow:
                assert r.temporal_light_motion_stats() == m.lf_stats, f"rt_temporal_light_motion_stats {r.temporal_light_motion_stats()}, the model {m.lf_stats}"


def setup(p, oracle, c, tris):
    opt = oracle.bench_options(**(dict(use_shadowed_target_function=1) if c.shape == "shadowed" else {}))
    p.set_scene(tris)
    p.set_options(opt)
    p.tuning(16, 0)  # primary rays never through the work-sharing walk: the whole frame's form at the benchmark size
    if c.shape.startswith("two launches"):
        p.tuning(25, 0)
    if c.shape == "two launches, no work sharing":
        p.tuning(13, 0)
    for k in c.exp:
        p.tuning(k, 1)
    if c.selection == "power":
        p.light_sampling("power")
    if c.selection == "grid":
        p.light_grid(*GRID)
    if c.history != "own pixel":
        p.temporal_reprojection(True)
    if c.history == "motion":
        p.temporal_motion(True)
    if c.t_unbiased:
        p.temporal_unbiased(True)
    if c.s_unbiased:
        p.spatial_unbiased(True)
    if c.follow:
        p.temporal_light_motion(True)
    p.walk_stats_enable(True)


def run(oracle, scenes, c, api=None):
    """the case through the model (and the device, with `api`); returns (launches predicted over the frames, the model)"""
    p = Pair(oracle, c.W, c.H, scenes, api=api, exp=bool(c.exp))
    try:
        t = start_scene()
        setup(p, oracle, c, t)
        launches = set()
        for k in range(FRAMES):
            if k and not c.exp:
                t = move(t, BOX_STEP, BOX_LO, BOX_HI - BOX_LO)
                p.update_scene(t, BOX_LO, BOX_HI - BOX_LO, "box")
                t = move(t, PANEL_STEP, P0, 2)
                p.update_scene(t, P0, 2, "panel")
            if not k or not c.exp:
                p.lookat(*orbit(ORBIT * k))
            if c.path == "kernels":
                launches |= set(p.kernels(1 + k))
            else:
                want = p.frame(1 + k)
                assert want.code == 0, (want, p.log)
                launches |= set(want.launches)
                if k == 0:
                    for r in p.r:
                        assert r.stage0_one_launch() == want.one_launch, f"rt_stage0_one_launch {r.stage0_one_launch()}, the model {want.one_launch}"
        p.check_stats()
        return launches, p.m
    finally:
        p.close()


def conditions(c, m):
    """the case really contains what it names: by the model alone"""
    s = m.seen
    if c.exp:
        return
    if c.history == "reproject":
        assert s["reprojected_from_another_pixel"] > 0, (case_id(c), s)
    if c.history == "motion":
        assert s["motion_valid"] > 0 and s["motion_elsewhere"] > 0, (case_id(c), s)
    if c.follow:
        assert s["records_moved"] > 0, (case_id(c), s)
    if c.t_unbiased:
        assert s["kept_out_of_z"] > 0, (case_id(c), s)


# --------------------------------------------------------------------------------------------------------------------- soak
# np.random.default_rng(SOAK_SEED + seed). 3500 .. 3510 each leave one of the four runs without one of SOAK_NEEDS (by the model alone);
# 3511 is the first constant under which all four hold all six
SOAK_SEED, SOAK_FRAMES = 3511, 32
SOAK_CASES = [(0, 37, 29), (1, 37, 29), (2, 37, 29), (0, 8, 8)]
GRIDS = [(0, 0), (16, 64), (4, 8), (2, 3)]
DIM = np.array([20.0, 18.0, 14.0], np.float32)
# the events, each as often as its weight: 0 nothing, 1 orbit, 2 box, 3 panel, 4 panel recoloured, 5 both moves, 6 a switch flips,
# 7 an option changes, 8 frame-number jump, 9 clear_first, 10 rt_raycast, 11 rt_raycast + rt_generate_candidate into RT_RES_1,
# 12 rt_resolve + rt_tone_mapping again, 13 a knob of context A flips. A switch flips most often: a uniform draw leaves 32 frames with
# two flips, and no seed then holds a motion launch, an unbiased launch and a refusal
EVENTS = np.repeat(np.arange(14), [2, 3, 2, 2, 1, 2, 8, 2, 1, 1, 1, 1, 1, 2])
# what every seed has to contain, by the model alone (tests/test_frame_model_cpu.py)
SOAK_NEEDS = ("reuse_frames", "motion_elsewhere", "records_moved", "unbiased_launches", "refused", "grid_frames_after_a_light_move")


def _knobs_off(p, r):
    """context B: every shortcut off"""
    r.gbuffer_reuse(False)
    r.occluder_hints(False)
    r.neighbour_pick(0)
    for key in (13, 14, 25):
        r.tuning(key, 0)


def soak(oracle, scenes, seed, W, H, api=None):
    """32 frames; between two frames zero, one or two events. Context A has default knobs (the model follows its primary-ray count),
    context B every shortcut off; both receive the same calls and hold the model's bytes after every frame. Returns the model."""
    rng = np.random.default_rng(SOAK_SEED + seed)
    p = Pair(oracle, W, H, scenes, api=api)
    if api:
        p.r.append(api.Renderer(W, H))
    A = p.r[:1]
    try:
        t = start_scene()
        opt = dict(use_shadowed_target_function=0, spatial_resampling_passes=3, accumulate=0)
        p.set_scene(t)
        p.set_options(oracle.bench_options(**opt))
        if api:
            _knobs_off(p, p.r[1])
        # the switches start in a random legal state
        on = dict(spatial_unbiased=False, light_sampling=False, temporal_reprojection=False, temporal_motion=False, temporal_unbiased=False,
                  temporal_light_motion=False, light_grid=0)
        for k in on:
            if k == "light_grid":
                on[k] = int(rng.integers(0, len(GRIDS)))
                p.light_grid(*GRIDS[on[k]])
            elif k == "light_sampling":
                on[k] = bool(rng.integers(0, 2))
                p.light_sampling("power" if on[k] else "uniform")
            elif rng.integers(0, 4) and not (k == "temporal_unbiased" and on["temporal_motion"]):
                on[k] = True
                getattr(p, k)(True)
        angle, n, dims, last_out = 0.0, 0, 0, None
        p.lookat(*orbit(angle))
        knobs = {13: 1, 14: -1, 17: -1, 25: -1, "gbuffer_reuse": 1, "occluder_hints": 1, "neighbour_pick": 1}

        def box():
            nonlocal t
            t = move(t, (0.0, 0.0, float(rng.choice([1.0, -1.0, 0.5]))), BOX_LO, BOX_HI - BOX_LO)
            p.update_scene(t, BOX_LO, BOX_HI - BOX_LO, "box")

        def panel():
            nonlocal t
            t = move(t, (float(rng.choice([0.3, -0.3])), 0.0, -0.1), P0, 2)
            p.update_scene(t, P0, 2, "panel")

        def switch(k, v):
            if on[k] != v:
                want = getattr(p, k)(v)
                if want is None or want.code == 0:
                    on[k] = v

        for f in range(SOAK_FRAMES):
            clear = False
            jump = 1
            # rt_temporal_motion and rt_temporal_unbiased refuse each other, and a uniform draw over seven switches leaves hardly a run of
            # 32 frames with launches of both (none of 60 constants tried did): the regime changes at three fixed frames, in calls that
            # are events like any other; everything between them is drawn
            if f == 8:
                switch("temporal_unbiased", False)
                switch("temporal_reprojection", True)
                switch("temporal_motion", True)
                switch("temporal_light_motion", True)
            if f == 16:
                if on["temporal_motion"]:
                    assert p.temporal_unbiased(True).code == fm.RT_ERR_UNSUPPORTED  # the second of the two is refused
                switch("temporal_motion", False)
                switch("temporal_unbiased", True)
            if f == 24 and on["light_grid"] == 0:
                on["light_grid"] = 1
                p.light_grid(*GRIDS[1])
            for _ in range(int(rng.integers(0, 3))):
                e = int(rng.choice(EVENTS))
                if e == 0:
                    p.log.append("nothing")
                elif e == 1:
                    angle += ORBIT
                    p.lookat(*orbit(angle))
                elif e == 2:
                    box()
                elif e == 3:
                    panel()
                elif e == 4:
                    dims += 1
                    t = t.copy()
                    t["emissive"][P0:P0 + 2] = (DIM * np.float32(0.85) ** dims).astype(np.float32)
                    p.update_scene(t, P0, 2, "panel recoloured")
                elif e == 5:
                    box()
                    panel()
                elif e == 6:
                    k = list(on)[int(rng.integers(0, len(on)))]
                    if k == "light_grid":
                        on[k] = (on[k] + 1 + int(rng.integers(0, len(GRIDS) - 1))) % len(GRIDS)
                        p.light_grid(*GRIDS[on[k]])
                    elif k == "light_sampling":
                        on[k] = not on[k]
                        p.light_sampling("power" if on[k] else "uniform")
                    else:
                        want = getattr(p, k)(not on[k])
                        if want is None or want.code == 0:
                            on[k] = not on[k]
                elif e == 7:
                    k = ("use_shadowed_target_function", "spatial_resampling_passes", "accumulate")[int(rng.integers(0, 3))]
                    opt[k] = 1 + (opt[k] % 3) if k == "spatial_resampling_passes" else 1 - opt[k]
                    p.set_options(oracle.bench_options(**opt))
                elif e == 8:
                    jump = int(rng.integers(2, 40))
                    p.log.append(f"frame number + {jump}")
                elif e == 9:
                    clear = True
                elif e == 10:
                    p.call("rt_raycast", lambda: p.m.raycast(), "rt_raycast")
                elif e == 11:
                    p.call("rt_raycast", lambda: p.m.raycast(), "rt_raycast")
                    want = p.call(f"rt_generate_candidate {n + 1} -> RES_1", lambda: p.m.generate_candidate(n + 1, 1), "rt_generate_candidate", n + 1, 1)
                    assert want.code == 0
                elif e == 12:
                    if last_out is not None and p.m.gbuffer_is_current():  # the G-buffer the records were resolved under
                        p.call(f"rt_resolve {last_out}", lambda: p.m.resolve(last_out), "rt_resolve", last_out)
                        p.call("rt_tone_mapping", lambda: p.m.tone_mapping(), "rt_tone_mapping")
                        p.check("resolve again", last_out)
                elif e == 13:
                    k = list(knobs)[int(rng.integers(0, len(knobs)))]
                    if isinstance(k, int):
                        knobs[k] = int(rng.choice({13: [0, 1], 14: [-1, 0, 1, 2], 17: [-1, 0, 1], 25: [-1, 0, 1]}[k]))
                        p.tuning(k, knobs[k], only=A)
                    else:
                        knobs[k] = int(rng.integers(0, 3 if k == "neighbour_pick" else 2))
                        p.log.append(f"{k} {knobs[k]} (A)")
                        getattr(p.m, k)(knobs[k])
                        for r in A:
                            getattr(r, k)(knobs[k])
            n += jump
            before = p.m.primary_launches
            base = [r.primary_launches() for r in A]
            want = p.frame(n, clear)
            if want.code == 0:
                last_out = want.out
            for r, b in zip(A, base):
                got = r.primary_launches() - b
                assert got == p.m.primary_launches - before, f"frame {n}: {got} launches traced primary rays, the model says {p.m.primary_launches - before}\n{p.log}"
        return p.m
    finally:
        p.close()
