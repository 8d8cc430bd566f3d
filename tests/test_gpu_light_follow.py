"""rt_temporal_light_motion on the device: k_light_follow (csrc/light_follow_kernels.h) against tests/light_follow_ref.py (the restatement
compiled from the kernel's own header and anchored by tests/test_light_follow_cpu.py, which locates by brute force over the span), bit
for bit: per update, on scenes that stress the point query of the old wide tree, over frame sequences, and the host rules of the toggle.

Sizes: 64 x 48 (whole tiles), 37 x 29 and 19 x 7 (partial tiles), 8 x 8 (one wavefront). Scene: the lamp room; its panel (triangles PANEL)
moves, grows, goes dark or stays."""
import ctypes as C

import numpy as np
import pytest

import bvh_build_scenes as S
import light_follow_ref as lf
import light_sampling_ref as ls
import temporal_reproject_ref as tr
from cedec_2024_rt_amd import scenes
from test_light_follow_cpu import ALL_LO, ALL_N, BASE, P0, Worlds, move, scale_panel
from test_temporal_reproject_cpu import FOVY, _orbit, _res_diff

pytestmark = pytest.mark.gpu

RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 1, 3, 5  # include/restir_rt.h
SIZES = [(8, 8), (19, 7), (37, 29), (64, 48)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def worlds(oracle):
    return Worlds(oracle)


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def _changed(kind):
    if kind == "moved":
        return move(BASE, (0.6, 0.0, -0.3))
    if kind == "scaled":
        return scale_panel(BASE, 1.25)
    if kind == "switched off":
        t = BASE.copy()
        t["emissive"][P0:P0 + 2] = 0
        return t
    if kind == "moved and dimmed":  # still emissive, another Ke: the stored luminance has to follow
        t = move(BASE, (0.6, 0.0, -0.3))
        t["emissive"][P0:P0 + 2] = np.array([12.5, 10.0, 7.5], np.float32)
        return t
    return BASE.copy()  # left alone


RES_SHADED_BIT, RES_M_MASK = 0x40000000, 0x3FFFFFFF  # csrc/rt_device.h


def _raw(r, res):
    """the buffer as it lies on the device (rt_halo_pack copies it): (n, 16) uint32 records {hit_p, ucw}{hit_n, M | flags}{origin_p, lum}
    {origin_n, w_sum} and (n, 4) uint32 side records {radiance, own-visibility word}: what the 76-byte download drops"""
    import torch

    n = r.W * r.H
    t = torch.zeros(80 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the copy below on the context's
    r.halo_pack(res, 0, r.H, t.data_ptr())
    r.sync()
    a = t.cpu().numpy()
    return a[:64 * n].view(np.uint32).reshape(n, 16).copy(), a[64 * n:].view(np.uint32).reshape(n, 4).copy()


def _luminance_bits(ke):
    """luminance(Ke) of csrc/rt_device.h in binary32, in its order"""
    k = np.asarray(ke, np.float32)
    c = np.array([0.1762044, 0.8129847, 0.0108109], np.float32)
    return np.array([np.float32(np.float32(k[0] * c[0]) + np.float32(k[1] * c[1])) + np.float32(k[2] * c[2])], np.float32).view(np.uint32)[0]


def _check_raw(raw_before, raw_after, before76, want76, located, new, shaded):
    """the three outputs of the rule that no download shows: the stored luminance, the word of M and flags, the own-visibility word"""
    (rb, sb), (ra, sa) = raw_before, raw_after
    changed = _bits(before76).reshape(len(before76), -1) != _bits(want76).reshape(len(want76), -1)
    changed = changed.any(axis=1)
    emptied = changed & (want76["M"] == 0)
    moved = changed & ~emptied
    keep = ~changed
    assert np.array_equal(ra[keep], rb[keep]) and np.array_equal(sa[keep], sb[keep]), "a record that was not carried changed a byte on the device"
    if moved.any():
        lum = np.array([_luminance_bits(new["emissive"][t]) for t in located[moved]], np.uint32)
        assert np.array_equal(ra[moved, 11], lum), "stored luminance is not luminance(Ke') of the new triangle"
        assert np.array_equal(ra[moved, 7], rb[moved, 7]), "M, the visibility flag and the shaded bit stay"
        assert (sa[moved, 3] == 0).all(), "the own-visibility word says nothing known"
        assert np.array_equal(ra[moved][:, [8, 9, 10, 12, 13, 14, 15]], rb[moved][:, [8, 9, 10, 12, 13, 14, 15]]), "origin and w_sum stay"
    if emptied.any():
        z = np.zeros(16, np.uint32)
        z[7] = RES_SHADED_BIT
        assert (ra[emptied] == z).all() and (sa[emptied] == 0).all(), "Reservoir{} with the shaded bit kept"
        assert ((rb[emptied, 7] & RES_SHADED_BIT) != 0).all()
    return int(moved.sum()), int(emptied.sum())


def _buffers(api, r):
    return {b: r.download(b) for b in (api.RT_BUF_RES_0, api.RT_BUF_RES_1, api.RT_BUF_RES_TEMPORAL)}


def _want(before, shaded, old, new, first, count):
    """the restatement on the shaded records (the kernel examines the shaded bit and M > 0); every other record keeps its bytes"""
    b = before.copy()
    b["M"][~shaded] = 0
    out, located, _, counts = lf.rebase(b, old, new, first, count)
    out[~shaded] = before[~shaded]
    return out, located, counts


def _shaded(api, r, tris):
    vis = r.download(api.RT_BUF_VISIBILITY)
    idx = vis["index"]
    return (idx >= 0) & ~(tris["emissive"] > 0).any(axis=1)[np.maximum(idx, 0)]


# ---------------------------------------------------------------------------------------------------------------- per update
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", ["moved", "scaled", "switched off", "left alone", "moved and dimmed"])
def test_an_update_equals_the_restatement(api, oracle, W, H, kind):
    r = api.Renderer(W, H)
    r.set_scene(BASE)
    r.set_options(oracle.bench_options())
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
    assert r.temporal_light_motion(True) == dict(on=True, rebased=0)
    r.frame(1)
    r.frame(2)
    shaded = _shaded(api, r, BASE)
    before = _buffers(api, r)
    raw_before = _raw(r, api.RT_RES_TEMPORAL)
    new = _changed(kind)
    r.update_scene(new[P0:P0 + 2], first=P0)
    after = _buffers(api, r)
    raw_after = _raw(r, api.RT_RES_TEMPORAL)
    n_buffers = r.temporal_light_motion()["rebased"]
    assert n_buffers in (3, 4), "the three logical buffers, and the fourth physical one the staged frame rotates through"
    total = dict(examined=0, located=0, moved=0, emptied=0)
    for b in before:
        want, located, counts = _want(before[b], shaded, BASE, new, P0, 2)
        assert after[b].tobytes() == want.tobytes(), f"{W} x {H} {kind}: buffer {b}: {_res_diff(after[b], want)}"
        for k in total:
            total[k] += counts[k]
    st = r.temporal_light_motion_stats()
    assert st["buffers"] == n_buffers and all(st[k] >= total[k] for k in total), (st, total)
    if n_buffers == 3:
        assert st == dict(buffers=3, **total), (st, total)
    assert total["located"] > 0
    want_t, located_t, _ = _want(before[api.RT_BUF_RES_TEMPORAL], shaded, BASE, new, P0, 2)
    n_moved, n_emptied = _check_raw(raw_before, raw_after, before[api.RT_BUF_RES_TEMPORAL], want_t, located_t, new, shaded)
    assert (n_moved > 0) == (kind in ("moved", "scaled", "moved and dimmed")) and (n_emptied > 0) == (kind == "switched off")
    if kind in ("moved", "scaled", "moved and dimmed"):
        assert total["moved"] == total["located"] and not _eq_bits(after[api.RT_BUF_RES_TEMPORAL], before[api.RT_BUF_RES_TEMPORAL])
    elif kind == "switched off":
        assert total["emptied"] == total["located"]
    else:
        assert total["moved"] == total["emptied"] == 0 and all(_eq_bits(after[b], before[b]) for b in before)
    r.close()


def test_buffers_that_do_not_qualify_are_unchanged(api, oracle):
    W, H = 37, 29
    r = api.Renderer(W, H)
    r.set_scene(BASE)
    r.set_options(oracle.bench_options())
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
    r.frame(1)
    a = move(BASE, (0.6, 0.0, 0.0))
    r.update_scene(a[P0:P0 + 2], first=P0)  # the toggle is off: this update is not followed, the buffers are now one generation old
    before = _buffers(api, r)
    r.temporal_light_motion(True)
    b = move(a, (0.6, 0.0, 0.0))
    r.update_scene(b[P0:P0 + 2], first=P0)
    assert r.temporal_light_motion() == dict(on=True, rebased=0)
    older = _buffers(api, r)
    assert all(_eq_bits(older[k], before[k]) for k in before), "a buffer one generation old changed"
    # one fresh buffer among older ones: only it is re-based, while the launches run the others keep every byte
    r.raycast()
    r.generate_candidate(5, api.RT_RES_0)
    shaded = _shaded(api, r, b)
    mixed = _buffers(api, r)
    c0 = move(b, (0.3, 0.0, 0.0))
    r.update_scene(c0[P0:P0 + 2], first=P0)
    assert r.temporal_light_motion()["rebased"] == 1
    got = _buffers(api, r)
    want0, _, counts0 = _want(mixed[api.RT_BUF_RES_0], shaded, b, c0, P0, 2)
    assert counts0["moved"] > 0 and got[api.RT_BUF_RES_0].tobytes() == want0.tobytes()
    assert _eq_bits(got[api.RT_BUF_RES_1], mixed[api.RT_BUF_RES_1]) and _eq_bits(got[api.RT_BUF_RES_TEMPORAL], mixed[api.RT_BUF_RES_TEMPORAL])
    b = c0
    # a span without a light re-bases nothing either, on fresh buffers
    r.frame(2)
    mid = _buffers(api, r)
    c = move(b, (0.0, 0.2, 0.0), 0, 4)
    r.update_scene(c[0:4], first=0)
    assert r.temporal_light_motion()["rebased"] == 0
    after = _buffers(api, r)
    assert all(_eq_bits(after[k], mid[k]) for k in mid)
    st = r.temporal_light_motion_stats()
    assert st == dict(buffers=1, **counts0)
    r.close()


# ------------------------------------------------------------------------------------------------------------- the point query
def _query_case(api, oracle, tris, eye, at, W, H, first, count, new, split=None, min_located=20):
    """candidates on `tris`, then the same update on two contexts' worth of paths: the old tree's point query and the direct loop;
    both equal the restatement's brute force"""
    got = {}
    for path in (0, 1 << 30):
        r = api.Renderer(W, H)
        if split is not None:
            r.bvh_config(split)
        r.set_scene(tris)
        r.set_options(oracle.bench_options())
        r.lookat(eye, at, fovy=FOVY)
        r.temporal_light_motion(True)
        r.temporal_light_motion_path(path)
        r.raycast()
        r.generate_candidate(3, api.RT_RES_0)
        shaded = _shaded(api, r, tris)
        before = r.download(api.RT_BUF_RES_0)
        others = {b: r.download(b) for b in (api.RT_BUF_RES_1, api.RT_BUF_RES_TEMPORAL)}
        r.update_scene(new[first:first + count], first=first)
        assert r.temporal_light_motion()["rebased"] == 1, "only the buffer the candidates were written to carries a tag"
        assert all(_eq_bits(r.download(b), others[b]) for b in others), "an untagged buffer changed while another was re-based"
        got[path] = (before, r.download(api.RT_BUF_RES_0), shaded, r.bvh_info(), r.temporal_light_motion_stats())
        r.close()
    before, after, shaded, info, st = got[0]
    assert _eq_bits(before, got[1 << 30][0])
    want, located, counts = _want(before, shaded, tris, new, first, count)
    assert counts["located"] >= min_located, f"only {counts['located']} records lie on the span: the case covers nothing"
    assert after.tobytes() == want.tobytes(), f"point query: {_res_diff(after, want)} of {counts}"
    assert got[1 << 30][1].tobytes() == want.tobytes(), f"direct loop: {_res_diff(got[1 << 30][1], want)}"
    assert st == dict(buffers=1, **counts) and got[1 << 30][4] == st, (st, got[1 << 30][4], counts)
    return counts, located, info


def _as_triangles(v, emissive_mask):
    from cedec_2024_rt_amd.types import TRIANGLE

    t = np.zeros(len(v), dtype=TRIANGLE)
    t["v"] = v.reshape(t["v"].shape)
    t["color"] = 0.8
    t["emissive"][emissive_mask] = np.float32(3.0)
    return t


def test_point_query_on_presplit_emissive_triangles(api, oracle):
    """tests/bvh_build_scenes.py 'large:66': a soup whose few large triangles the default split factor cuts into fragments, one leaf
    each. The large triangles and every eighth other one are emissive; all of them move"""
    v, _, split = S.scene("large:66")
    v = np.array(v)
    ext = (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    large = ext > 10 * np.median(ext)
    assert 1 <= large.sum() <= 4
    em = large | (np.arange(len(v)) % 8 == 0)
    tris = _as_triangles(v, em)
    new = move(tris, (0.3, -0.2, 0.1), 0, len(tris))
    counts, located, info = _query_case(api, oracle, tris, (0.0, 0.3, 2.5), (0.0, 0.0, 0.0), 64, 48, 0, len(tris), new, split=split)
    assert np.isin(located[located >= 0], np.where(large)[0]).sum() >= 10, "no record on a pre-split triangle"
    assert info["references"] > len(tris), "nothing was split: the case covers no fragments"


def test_point_query_on_the_blocks_stand_in(api, oracle):
    """the whole light span of the bench stand-in (thinned foliage) at 64 x 36: thousands of span lights, a walk of several levels"""
    tris = scenes.make_blocks_restir(detail=0.25)
    lights = scenes.light_indices(tris)
    first, count = int(lights.min()), int(lights.max()) + 1 - int(lights.min())
    assert len(lights) > 1000
    new = move(tris, (0.0, 0.25, 0.0), first, count)
    counts, located, info = _query_case(api, oracle, tris, scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT, 64, 36, first, count, new, min_located=500)
    assert info["wide_height"] >= 4 and len(np.unique(located[located >= 0])) > 100


def test_point_query_with_lights_flush_with_coplanar_geometry(api, oracle):
    """the panel's two triangles doubled by non-emissive triangles of the same vertices inside the span, and a non-emissive sheet in the
    panel's plane around it: the exact test separates them by their radiance"""
    t = np.concatenate([BASE[:P0 + 2], BASE[P0:P0 + 2], BASE[P0:P0 + 2], BASE[P0 + 2:]])
    t["emissive"][P0 + 2:P0 + 4] = 0  # the doubles
    t["emissive"][P0 + 4:P0 + 6] = 0  # the sheet: the panel's plane, four times the size
    c = t["v"][P0 + 4:P0 + 6].reshape(-1, 3).astype(np.float64).mean(axis=0)
    t["v"][P0 + 4:P0 + 6] = (c + (t["v"][P0 + 4:P0 + 6].astype(np.float64).reshape(-1, 3) - c) * 2.0).astype(np.float32).reshape(t["v"][P0 + 4:P0 + 6].shape)
    new = move(t, (0.5, 0.0, 0.5), P0, 6)
    counts, located, _ = _query_case(api, oracle, t, ls.LAMP_EYE, ls.LAMP_AT, 37, 29, P0, 6, new)
    assert set(np.unique(located[located >= 0])) <= {P0, P0 + 1}


# ----------------------------------------------------------------------------------------------------------------- sequences
FRAMES, STEP, ORBIT = 6, (0.3, 0.0, -0.1), 0.1


class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU with one scene and one camera per frame: the oracle's kernels; before a frame
    whose scene differs from the last one's the history is re-based by the restatement; with `reproject` the temporal merge is
    tests/temporal_reproject_ref.py's"""

    def __init__(self, oracle, W, H, opt, follow, reproject):
        self.o, self.W, self.H, self.opt, self.follow, self.reproject = oracle, W, H, opt, follow, reproject
        self.st = oracle.new_state(W, H)
        self.prev = None

    def frame(self, frame, world, view):
        sc, st, W, H, opt = world["scene"], self.st, self.W, self.H, self.opt
        st["vis"] = view.vis
        if self.prev is not None and self.follow:
            st["temporal"][:] = lf.rebase(st["temporal"], self.prev[0]["tris"], world["tris"], P0, 2)[0]
        sc.generate_candidate(W, H, frame, view.vis, view.eye, opt, st["r0"])
        if self.prev is None or not self.reproject:
            sc.temporal_resampling(W, H, frame, view.vis, view.eye, opt, st["temporal"], st["r0"])
        else:
            pv = self.prev[1]
            tr.temporal(W, H, frame, world["tris"], view.vis, pv.vis, view.eye, pv.rg, view.rg, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        self.prev = (world, view)
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            st[dst] = sc.spatial_resampling(W, H, frame, k, view.vis, view.eye, opt, st[src])
        sc.resolve(st["accum"], W, H, view.vis, view.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _dim(t, k):
    """the panel recoloured and dimmed a little more with every frame, still emissive"""
    t = t.copy()
    t["emissive"][P0:P0 + 2] = (np.array([20.0, 18.0, 14.0], np.float32) * np.float32(0.85) ** k).astype(np.float32)
    return t


@pytest.mark.parametrize("W,H,orbit,reproject,follow,dim", [(37, 29, False, False, True, False), (37, 29, True, True, True, False), (64, 48, True, False, True, False),
                                                            (19, 7, False, True, True, False), (37, 29, False, False, False, False),
                                                            (37, 29, False, False, True, True), (19, 7, True, True, True, True)])
def test_frames_with_a_moving_panel_equal_the_cpu_sequence(api, oracle, worlds, W, H, orbit, reproject, follow, dim):
    opt = oracle.bench_options()
    cpu = _Cpu(oracle, W, H, opt, follow, reproject)
    r = api.Renderer(W, H)
    r.set_scene(BASE)
    r.set_options(opt)
    if reproject:
        r.temporal_reprojection(True)
    r.temporal_light_motion(follow)
    t = BASE
    moved = 0
    for k in range(FRAMES):
        if k:
            t = move(t, STEP)
            if dim:  # the next frame's merge reads the stored luminance: a stale one shows in its records
                t = _dim(t, k)
            r.update_scene(t[P0:P0 + 2], first=P0)
            assert r.temporal_light_motion()["rebased"] in ((3, 4) if follow else (0,))
        w = worlds.of(t)
        view = worlds.view_at(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT * k if orbit else 0.0))
        r.lookat(view.eye, view.at, fovy=FOVY)
        out = r.frame(1 + k)
        last = cpu.frame(1 + k, w, view)
        what = f"frame {1 + k}"
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation"
        assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
        assert not _res_diff(r.download(api.RT_BUF_RES_0 + out), last, view.shaded), f"{what}: records"
        assert not _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], view.shaded), f"{what}: temporal history"
    if follow:
        moved = r.temporal_light_motion_stats()["moved"]
        assert moved > 0
    r.close()


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_two_light_updates_with_no_frame_between_them(api, oracle, W, H):
    """light_gen chains on the host: the second update finds the samples where the first put them, a third after an update that was
    not followed finds nothing to re-base"""
    r = api.Renderer(W, H)
    r.set_scene(BASE)
    r.set_options(oracle.bench_options())
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
    r.temporal_light_motion(True)
    r.frame(1)
    shaded = _shaded(api, r, BASE)
    before = _buffers(api, r)
    a = move(BASE, (0.6, 0.0, 0.0))
    b = scale_panel(move(a, (0.0, -0.25, 0.5), ALL_LO, ALL_N), 1.25)
    r.update_scene(a[P0:P0 + 2], first=P0)
    n1 = r.temporal_light_motion()["rebased"]
    r.update_scene(b[ALL_LO:ALL_LO + ALL_N], first=ALL_LO)
    n2 = r.temporal_light_motion()["rebased"]
    assert n1 in (3, 4) and n2 == n1
    after = _buffers(api, r)
    moved = 0
    for k in before:
        w1, _, _ = _want(before[k], shaded, BASE, a, P0, 2)
        w2, _, c2 = _want(w1, shaded, a, b, ALL_LO, ALL_N)
        assert after[k].tobytes() == w2.tobytes(), f"buffer {k}: {_res_diff(after[k], w2)}"
        moved += c2["moved"]
    assert moved > 0
    r.temporal_light_motion(False)
    c = move(b, (0.1, 0.0, 0.0))
    r.update_scene(c[P0:P0 + 2], first=P0)
    r.temporal_light_motion(True)
    d = move(c, (0.1, 0.0, 0.0))
    r.update_scene(d[P0:P0 + 2], first=P0)
    assert r.temporal_light_motion()["rebased"] == 0
    assert all(_eq_bits(r.download(k), after[k]) for k in after)
    r.close()


# ------------------------------------------------------------------------------------------------------ toggle off, host rules
def test_toggle_off_is_the_parent(api, oracle):
    """two contexts, one that never heard of the toggle and one that had it on and off again: same bytes, primary launches and walk counters"""
    W, H = 37, 29
    out = []
    for touch in (False, True):
        r = api.Renderer(W, H)
        r.set_scene(BASE)
        r.set_options(oracle.bench_options())
        r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
        if touch:
            r.temporal_light_motion(True)
            r.temporal_light_motion(False)
        r.walk_stats_enable(True)
        t = BASE
        for k in range(3):
            if k:
                t = move(t, STEP)
                r.update_scene(t[P0:P0 + 2], first=P0)
                assert r.temporal_light_motion()["rebased"] == 0
            r.frame(1 + k)
        out.append((_buffers(api, r), r.download(api.RT_BUF_ACCUMULATION), r.download(api.RT_BUF_PIXELS), r.primary_launches(), r.walk_stats()))
        r.close()
    a, b = out
    assert all(_eq_bits(a[0][k], b[0][k]) for k in a[0]) and _eq_bits(a[1], b[1]) and _eq_bits(a[2], b[2])
    assert a[3] == b[3] and a[4] == b[4]


def test_host_rules(api, oracle):
    r = api.Renderer(16, 12)
    L, h = r.L, r.h
    on, n, ms = C.c_int(-1), C.c_int(-1), C.c_float()
    st = np.zeros(5, np.uint64)
    assert L.rt_temporal_light_motion_get(h, C.byref(on), C.byref(n)) == 0 and (on.value, n.value) == (0, 0)
    assert L.rt_temporal_light_motion_get(h, None, None) == RT_ERR_ARG
    assert L.rt_temporal_light_motion_get(h, C.byref(on), None) == 0 and L.rt_temporal_light_motion_get(h, None, C.byref(n)) == 0
    assert L.rt_temporal_light_motion_stats(h, None) == RT_ERR_ARG
    assert L.rt_temporal_light_motion_stats(h, st.ctypes.data_as(C.c_void_p)) == RT_ERR_STATE, "never on: no totals"
    assert L.rt_temporal_light_motion_timing(h, None) == RT_ERR_ARG
    assert L.rt_temporal_light_motion_timing(h, C.byref(ms)) == RT_ERR_STATE
    assert L.rt_temporal_light_motion(None, 1) == RT_ERR_ARG
    # the toggle changes rt_state_epoch, before and after a scene, and touches no buffer
    e0 = _epoch(r)
    assert r.temporal_light_motion(True)["on"] is True and _epoch(r) > e0
    r.set_scene(BASE)
    r.set_options(oracle.bench_options())
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
    r.frame(1)
    before = _buffers(api, r)
    e1 = _epoch(r)
    assert r.temporal_light_motion(False)["on"] is False and _epoch(r) > e1
    assert r.temporal_light_motion(True)["on"] is True
    assert all(_eq_bits(before[k], r.download(k)) for k in before)
    assert r.temporal_light_motion_stats() == dict(buffers=0, examined=0, located=0, moved=0, emptied=0)
    # independent of the other toggles
    r.temporal_reprojection(True)
    r.temporal_motion(True)
    assert r.temporal_light_motion()["on"] is True
    r.temporal_motion(False)
    r.temporal_unbiased(True)
    r.spatial_unbiased(True)
    r.light_sampling("power")
    assert r.temporal_light_motion()["on"] is True
    # timing: only for an update under rt_timing_enable
    t = move(BASE, STEP)
    r.update_scene(t[P0:P0 + 2], first=P0)
    assert L.rt_temporal_light_motion_timing(h, C.byref(ms)) == RT_ERR_STATE
    r.frame(2)
    r.timing_enable(True)
    t = move(t, STEP)
    r.update_scene(t[P0:P0 + 2], first=P0)
    assert r.temporal_light_motion_timing() > 0.0
    r.update_scene(t[0:2], first=0)  # no light in the span: timed, nothing launched
    assert r.temporal_light_motion_timing() == 0.0
    # the totals restart when the toggle goes on again
    assert r.temporal_light_motion_stats()["buffers"] >= 3
    r.temporal_light_motion(False)
    r.temporal_light_motion(True)
    assert r.temporal_light_motion_stats()["buffers"] == 0
    r.close()


def test_strip_contexts_are_refused(api):
    r = api.Renderer(16, 12, rows=(0, 6))
    assert r.L.rt_temporal_light_motion(r.h, 1) == RT_ERR_UNSUPPORTED
    assert r.L.rt_temporal_light_motion(r.h, 0) == RT_ERR_UNSUPPORTED
    r.close()
