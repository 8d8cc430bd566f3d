"""CPU. The restatement of a followed rt_denoise_temporal call (tests/denoise_motion_ref.py: csrc/denoise_motion.h and the kernels'
other headers, equal to the GPU bit for bit) against the independent float64 statement of tests/denoise_motion_spec.py, which shares
no code with them: the bit-for-bit tests cannot see a wrong formula in the shared headers, this can.

Teacher-forced: every call of the statement gets the restatement's previous state, previous vertices, range and previous eye.
Tolerance as in tests/test_denoise_spec_cpu.py, from the statement alone: spread = its float32 run against its float64 run,
tol = 8 x spread, and tol <= 1e-4 or the input counts as ill-conditioned. Pixels whose float64 values sit within 1e-4 of a discrete
decision (the seven of tests/denoise_spec.py, each on the lookup point) are left out, at most 2 % of a call's participating pixels;
h is exact on all others.

Sequences on the lamp room at 40 x 33 and 64 x 48, four calls each: the box forward by 1 per call under a still camera, and the box
by (0.4, 0, 0.3) per call under an orbit of 0.1 rad per call."""
import ast
import os

import numpy as np
import pytest

import denoise_motion_ref as dm
import denoise_motion_spec as ms
import denoise_spec_cases as cs
import light_sampling_ref as ls
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, Worlds, move, on_box
from test_temporal_reproject_cpu import _orbit

SEQUENCES = {"forward_still": (MOVES[0], 0.0), "oblique_orbit": (MOVES[1], 0.1)}
CALLS = 4


@pytest.fixture(scope="module")
def worlds(oracle):
    return Worlds(oracle)


def test_the_statement_is_independent():
    """denoise_motion_spec imports numpy alone and neither opens a file nor loads a library"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_motion_spec.py")) as f:
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


@pytest.mark.parametrize("name", list(SEQUENCES))
@pytest.mark.parametrize("W,H", [(40, 33), (64, 48)])
def test_followed_calls_equal_the_float64_statement(worlds, W, H, name):
    offset, orbit = SEQUENCES[name]
    t = move(worlds.base, tuple(np.asarray(offset, np.float32) * np.float32(1 - CALLS)))
    M = dm.MotionRef(W, H, t, on=True, iterations=0)
    worst = {}
    for k in range(1, CALLS + 1):
        t = move(t, offset)
        M.update(t[BOX_LO:BOX_HI], BOX_LO)
        v = worlds.view(worlds.of(t), W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, orbit * (k - 1)))
        acc = cs.accumulation(W, H, 1000 * W + k, empty_seed=7, blocks=W > 40)
        prev = cs.prev_state(M)
        motion = dict(tris_prev=M.tv_prev.copy(), lo=M.lo, hi=M.hi, eye_prev=M.dt_eye.copy())
        _, mom = M(v.vis, v.eye, v.rg, acc)
        if prev is None:
            assert not M.followed
            continue
        assert M.followed
        rg9 = np.concatenate([np.asarray(v.rg[key], np.float32).reshape(3) for key in ("origin", "right", "up")])
        r64 = ms.temporal_stage(W, H, t, v.vis, v.eye, rg9, acc, prev, motion)
        r32 = ms.temporal_stage(W, H, t, v.vis, v.eye, rg9, acc, prev, motion, dtype=np.float32)
        part = r64["part"]
        box = on_box(v) & part
        assert np.array_equal(r64["on_range"], M.diag[:, 0] == 1) and np.array_equal(box, r64["on_range"]) and box.sum() >= 20
        left = part & (r64["margin"] < cs.MARGIN_MIN)
        share = float(left.sum()) / int(part.sum())
        assert share <= cs.LEFT_OUT_MAX, f"{name} {W} x {H} call {k}: {share:.3%} of the participating pixels sit on a decision"
        keep = part & ~left
        bad = keep & (mom[:, 2] != r64["moments"][:, 2])
        assert not bad.any(), f"{name} {W} x {H} call {k}: h differs on {int(bad.sum())} pixels, e.g. {int(np.flatnonzero(bad)[0])}"
        assert (mom[~part] == 0).all()
        assert (mom[keep & box, 2] == k).mean() > 0.75, "the box keeps its history"
        figs = [cs.check(f"{name} {W} x {H} call {k} {what}", cs.worst(cs.scalar_error(mom[:, j], r64["moments"][:, j]), keep),
                         cs.worst(cs.scalar_error(r32["moments"][:, j], r64["moments"][:, j]), keep)) for j, what in ((0, "mu1"), (1, "mu2"))]
        figs.append(cs.check(f"{name} {W} x {H} call {k} colour", cs.worst(cs.colour_error(M.hcol, r64["colour"]), keep),
                             cs.worst(cs.colour_error(r32["colour"], r64["colour"]), keep)))
        for f in figs:
            key = f["name"].split()[-1]
            if key not in worst or f["tol"] > worst[key]["tol"]:
                worst[key] = f
        worst["share"] = max(worst.get("share", 0.0), share)
    for key in ("mu1", "mu2", "colour"):
        f = worst[key]
        print(f"{f['name']}: error {f['err']:.3g} spread {f['spread']:.3g} tol {f['tol']:.3g}")
    print(f"{name} {W} x {H}: left out at most {worst['share']:.4%}")
