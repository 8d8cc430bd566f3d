"""CPU. The restatement of an adapted rt_denoise_temporal call (tests/denoise_antilag_ref.py: csrc/denoise_antilag.h and the kernels'
other headers, equal to the GPU bit for bit) against the independent float64 statement of tests/denoise_antilag_spec.py, which shares
no code with them: the bit-for-bit tests cannot see a wrong formula in the shared headers, this can.

Teacher-forced: every call of the statement gets the restatement's previous state (and, under follow-motion, its previous vertices,
range and previous eye), and is compared at 0, 1 and 2 iterations. Tolerance as in tests/test_denoise_spec_cpu.py, from the statement
alone: spread = its float32 run against its float64 run, tol = 8 x spread, and tol <= 1e-4 or the input counts as ill-conditioned.
h is exact. lambda' is compared absolutely (it is a blend weight in [0, 1], and 0 on most pixels); moments, colour history and image
relatively, as in the other spec tests.

Left out: the window's membership test n . n' >= 0.9 is the one new discrete decision. A pixel is left out if a candidate of its window
(a participating pixel with a history) is within 1e-4 of that threshold, or if any pixel of its window is within 1e-4 of one of the
lookup's decisions (which decide whether that pixel has a history, and its l_h); everything within the filter's reach of a left-out
pixel is left out of the colour history and the image. At most 2 % of a call's participating pixels. The scenes' normals meet at 0,
4 (the ring's facets), 15, 30 and 90 degrees, so the membership test itself leaves out nothing: asserted.

Scenes: the lamp room with its box moving under follow-motion (still camera and orbit), the faceted scene of
tests/denoise_spec_cases.py (creases of 15 and 30 degrees) under a sideways camera, and the wall and box of
tests/test_denoise_temporal_cpu.py under sideways steps. The accumulation is denoise_spec_cases' noise times a ramp across the image
whose slope changes from call to call, so that lambda spans the response's ramp and its lower clamp in every call.

Measured (printed by the tests; worst over all sequences, error of the restatement / spread / tol = 8 x spread, bar 1e-4):
  lambda' (absolute)          7.6e-7 / 7.6e-7 / 6.0e-6  (creases, radius 4, call 3)
  mu1                         4.1e-6 / 4.1e-6 / 3.3e-5  (the box by (0.4, 0, 0.3) under the orbit, 40 x 33, call 3)
  mu2                         1.06e-5 / 1.06e-5 / 8.5e-5  (the same call)
  colour history              4.5e-6 / 4.5e-6 / 3.6e-5  (the box forward under a still camera, 40 x 33, call 4, 2 iterations)
  image at 0 / 1 / 2 iterations  4.5e-6 / 4.5e-6 / 3.6e-5  (the same sequence, call 4, 1 iteration)
  left out: no pixel of any call (cap 2 %); h and the windows' member counts exact.
"""
import ast
import os

import numpy as np
import pytest

import denoise_antilag_ref as da
import denoise_antilag_spec as sp
import denoise_spec_cases as cs
import light_sampling_ref as ls
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, Worlds, move
from test_temporal_reproject_cpu import _orbit

AL = dict(radius=3, gradient_lo=0.2, gradient_hi=0.8, floor=0.1)
SLOPES = (0.0, 1.5, -0.55, 0.8, -0.3)  # per call: the accumulation is scaled by 1 + slope * x / W
ITERATIONS = (0, 2, 1)  # the last one leaves the state for the next call


@pytest.fixture(scope="module")
def worlds(oracle):
    return Worlds(oracle)


def test_the_statement_is_independent():
    """denoise_antilag_spec imports numpy alone and neither opens a file nor loads a library"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_antilag_spec.py")) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            imported.add((node.module or ".").split(".")[0])
        elif isinstance(node, ast.Call):
            name = node.func.id if isinstance(node.func, ast.Name) else getattr(node.func, "attr", "")
            assert name not in ("open", "exec", "eval", "__import__", "CDLL", "LoadLibrary", "fromfile", "load", "loadtxt", "genfromtxt", "memmap"), name
    assert imported == {"numpy"}, imported


def _accumulation(W, H, k, blocks):
    acc = cs.accumulation(W, H, 1000 * W + k, empty_seed=7, blocks=blocks)
    ramp = (1.0 + SLOPES[(k - 1) % len(SLOPES)] * (np.tile(np.arange(W), H) / W)).astype(np.float32)
    acc[:, :3] *= ramp[:, None]
    return acc


_STATE = ("has", "gx", "gn", "hcol", "hmom", "rg", "dt_gen", "dt_eye", "dt_dirty")


def _abs_error(a, ref):
    return np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))


def _compare(name, A, frames, al=AL):
    """frames: per call (tris, vis, eye, rg9-able rg, update or None). Returns the worst figure per quantity."""
    worst, shares, fired = {}, [], 0
    W, H = A.W, A.H
    for k, (t, vis, eye, rg, acc) in enumerate(frames, start=1):
        if k > 1:
            A.update(t[BOX_LO:BOX_HI], BOX_LO)
        prev = cs.prev_state(A)
        motion = dict(tris_prev=A.tv_prev.copy(), lo=A.lo, hi=A.hi, eye_prev=A.dt_eye.copy()) if A.on and A.tv_prev is not None else None
        saved = {s: getattr(A, s) for s in _STATE}
        rg9 = np.concatenate([np.asarray(rg[key], np.float32).reshape(3) for key in ("origin", "right", "up")])
        for it in ITERATIONS:
            for s, val in saved.items():
                setattr(A, s, val)
            out, mom = A(vis, eye, rg, acc, iterations=it)
            if prev is None:
                assert not A.adapted
                continue
            assert A.adapted and A.followed == (motion is not None)
            m = motion if A.followed else None
            r64 = sp.call(W, H, t, vis, eye, rg9, acc, prev, antilag=al, motion=m, iterations=it)
            r32 = sp.call(W, H, t, vis, eye, rg9, acc, prev, antilag=al, motion=m, iterations=it, dtype=np.float32)
            part = r64["part"]
            assert np.array_equal(part, r32["part"]) and part.sum() > W * H // 3
            assert not (r64["member_margin"] < cs.MARGIN_MIN).any(), "the scene puts a window's normal pair on the threshold"
            left = part & (cs._dilate(part & (r64["margin"] < cs.MARGIN_MIN), W, H, al["radius"]) | (r64["member_margin"] < cs.MARGIN_MIN))
            share = float(left.sum()) / int(part.sum())
            shares.append(share)
            assert share <= cs.LEFT_OUT_MAX, f"{name} call {k}: {share:.3%} of the participating pixels are left out"
            keep = part & ~left
            bad = keep & (mom[:, 2] != r64["moments"][:, 2])
            assert not bad.any(), f"{name} call {k}: h differs on {int(bad.sum())} pixels, e.g. {int(np.flatnonzero(bad)[0])}"
            assert (mom[~part] == 0).all()
            both = keep & r64["has"]
            assert np.array_equal(A.grad[both, 2].astype(np.int64), r64["members"][both]), f"{name} call {k}: member counts differ"
            tag = f"{name} call {k}, {it} iterations"
            figs = [cs.check(f"{tag} lambda'", cs.worst(_abs_error(mom[:, 3], r64["moments"][:, 3]), keep),
                             cs.worst(_abs_error(r32["moments"][:, 3], r64["moments"][:, 3]), keep))]
            figs += [cs.check(f"{tag} {what}", cs.worst(cs.scalar_error(mom[:, j], r64["moments"][:, j]), keep),
                              cs.worst(cs.scalar_error(r32["moments"][:, j], r64["moments"][:, j]), keep)) for j, what in ((0, "mu1"), (1, "mu2"))]
            kh = part & ~cs._dilate(left, W, H, 0 if it == 0 else 2 + 3)
            ko = part & ~cs._dilate(left, W, H, 0 if it == 0 else 2 * sum(1 << i for i in range(it)) + 3)
            assert (A.hcol[~part, 3] == -1).all()
            figs.append(cs.check(f"{tag} history", cs.worst(cs.colour_error(A.hcol, r64["history"]), kh), cs.worst(cs.colour_error(r32["history"], r64["history"]), kh)))
            figs.append(cs.check(f"{tag} hdr", cs.worst(cs.colour_error(out, r64["hdr"]), ko), cs.worst(cs.colour_error(r32["hdr"], r64["hdr"]), ko)))
            assert np.array_equal(out[~part].view(np.uint32), acc[~part].view(np.uint32))
            for f in figs:
                key = f["name"].split()[-1]
                if key not in worst or f["tol"] > worst[key]["tol"]:
                    worst[key] = f
            lr = r64["moments"][keep, 3]
            fired += int(((lr > 0) & (lr < 1)).sum())
            assert (lr == 0).any() and ((lr > 0) & (lr < 1)).sum() >= 20, f"{tag}: the input does not span the response"
    for key, f in worst.items():
        print(f"{f['name']}: error {f['err']:.3g} spread {f['spread']:.3g} tol {f['tol']:.3g}")
    print(f"{name}: left out at most {max(shares):.4%}; {fired} comparisons with 0 < lambda' < 1")
    return worst


@pytest.mark.parametrize("name", ["forward_still", "oblique_orbit"])
@pytest.mark.parametrize("W,H", [(40, 33), (64, 48)])
def test_followed_adapted_calls_equal_the_float64_statement(worlds, W, H, name):
    """MOTION x ANTILAG on the lamp room: the box moves before every call, the history follows it, and the window gradient reads the
    followed lookup's colour history"""
    offset, orbit = {"forward_still": (MOVES[0], 0.0), "oblique_orbit": (MOVES[1], 0.1)}[name]
    calls = 4
    t = move(worlds.base, tuple(np.asarray(offset, np.float32) * np.float32(1 - calls)))
    t = move(t, offset)
    A = da.AntilagRef(W, H, t, on=True, antilag=True, al=AL)
    frames = []
    for k in range(1, calls + 1):
        if k > 1:
            t = move(t, offset)
        v = worlds.view(worlds.of(t), W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, orbit * (k - 1)))
        # the empty records form blocks at both sizes: scattered ones leave pixels whose heaviest tap alone is invalid, where the float32
        # pixel coordinate's error is divided by the little weight that is left (tests/test_denoise_spec_cpu.py); with an accumulation
        # that changes from call to call that input measures tol 1.06e-4 at 40 x 33 under the orbit, above the bar
        frames.append((t, v.vis, v.eye, v.rg, _accumulation(W, H, k, True)))
    _compare(f"{name} {W} x {H}", A, frames)


@pytest.mark.parametrize("radius", [1, 4])
def test_creases_of_15_and_30_degrees_under_a_sideways_camera(oracle, radius):
    """the faceted scene of tests/denoise_spec_cases.py: facets 4 degrees apart and creases on either side of the threshold"""
    W, H = 40, 33
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = cs.scene()
    sc = oracle.Scene(tris, use_bvh=True)
    al = dict(AL, radius=radius)
    A = da.AntilagRef(W, H, tris, antilag=True, al=al)
    frames = []
    for k, pose in enumerate(cs.sequence("sideways", W, H), start=1):
        rg = cs.raygen(oracle, pose, W, H)
        frames.append((tris, sc.raycast(W, H, rg), pose[0], rg, _accumulation(W, H, k, False)))
    A.update = lambda *a: None  # nothing moves here
    _compare(f"creases radius {radius}", A, frames, al)


def test_wall_and_box_under_sideways_steps(oracle):
    """the wall and box of tests/test_denoise_temporal_cpu.py (normals at 0 and 90 degrees): disoccluded wall pixels have no history and
    are no members of their neighbours' windows"""
    from test_denoise_temporal_cpu import _wall_and_box

    W, H = 64, 36
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = _wall_and_box()
    sc = oracle.Scene(tris, use_bvh=True)
    A = da.AntilagRef(W, H, tris, antilag=True, al=AL)
    frames = []
    for k, x in enumerate((0.0, 0.5, 0.9, 0.4), start=1):
        eye, at = (x, 0.0, 2.0), (x, 0.0, -6.0)
        rg = oracle.raygen_lookat(eye, at, (0, 1, 0), cs.FOVY, W, H)
        frames.append((tris, sc.raycast(W, H, rg), eye, rg, _accumulation(W, H, k, True)))
    A.update = lambda *a: None
    _compare("wall and box", A, frames)
    assert (A.hmom[:, 2] == 1.0).any(), "no disoccluded pixel"
