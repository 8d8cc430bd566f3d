"""CPU. The C++ restatements of both denoisers (tests/denoise_ref.py, tests/denoise_temporal_ref.py: the loops restated, every
formula from csrc/denoise_math.h, equal to the GPU bit for bit) against the independent float64 reference of tests/denoise_spec.py,
which shares no code with them. The bit-for-bit tests cannot see a wrong formula in the shared header; these can.

Tolerance, per case and from the reference alone: spread = the float32 run of the reference against its float64 run on the same
input, tol = 8 * spread (summation order over up to 49 taps, pm_expf and sqrt_guarded against numpy's, up to 8 compounded
levels), and tol <= 1e-4 or the input counts as ill-conditioned. Inputs: tests/denoise_spec_cases.py.

Measured (worst over the cases; error of the restatement / spread / tol):
  spatial, 5 sizes x 4 iteration counts x 2 parameter sets:  4.1e-6 / 3.5e-6 / 2.8e-5 (spread and tol: 40 x 33, defaults, 5 and 8 iterations)
  temporal moments, 40 x 33 and 96 x 64, all sequences:      9.4e-6 / 9.4e-6 / 7.5e-5 (mu2, sideways at 40 x 33)
  temporal colour history:                                   2.6e-6 / 2.6e-6 / 2.1e-5 (turn at 40 x 33)
  temporal HDR at 0 / 1 / 2 iterations:                      2.4e-6 / 2.9e-6 / 2.3e-5 (static at 96 x 64)
  left out for a decision margin below 1e-4: at most 0.02 % of a call's participating pixels (cap 2 %); h exact on all others.
Each of sixteen errors planted in csrc/denoise_math.h ("Tests") fails this file by >= 1200 x tol or by an
exact h mismatch. On the static sequences every call is compared at 1 iteration and the calls of STATIC_FULL at 0 and 2 as well.
"""
import ast
import os

import numpy as np
import pytest

import denoise_ref
import denoise_spec_cases as cs
import denoise_temporal_ref as dtr

SIZES = [(64, 36), (40, 33), (19, 7), (7, 19), (8, 8)]
PARAMS = {"defaults": {}, "other": cs.OTHER}
# static sequences compare 0 and 2 iterations as well on these calls: around h = 4 (the temporal variance), h = 1 / alpha
# (5 and 20: the floor max(alpha, 1 / h) crosses alpha) and h = 32 (the cap)
STATIC_FULL = {1, 2, 3, 4, 5, 6, 19, 20, 21, 31, 32, 33, 34, 36}


@pytest.fixture(scope="module")
def world(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = cs.scene()
    return dict(ob=oracle, tris=tris, sc=oracle.Scene(tris, use_bvh=True), spatial={})


def _spatial_case(world, W, H):
    if (W, H) not in world["spatial"]:
        rg = cs.raygen(world["ob"], (cs.EYE, cs.AT), W, H)
        vis = world["sc"].raycast(W, H, rg)
        world["spatial"][W, H] = cs.SpatialCase(W, H, world["tris"], vis, cs.EYE, rg, cs.accumulation(W, H, 100 + W))
    return world["spatial"][W, H]


def test_the_reference_is_independent():
    """denoise_spec imports numpy alone and neither opens a file nor loads a library"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_spec.py")
    with open(path) as f:
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


@pytest.mark.parametrize("W,H", SIZES)
def test_the_scene_has_every_pixel_class(world, W, H):
    case = _spatial_case(world, W, H)
    index = case.vis["index"]
    tris = world["tris"]
    emissive = (tris["emissive"] > 0).any(axis=1)
    zero_albedo = (tris["color"] == 0).any(axis=1)
    hit = index >= 0
    assert (~hit).sum() >= 1, "no sky"
    assert emissive[index[hit]].sum() >= 1, "no emissive pixel"
    assert zero_albedo[index[hit]].sum() >= 2, "no pixel with a zero albedo channel"
    assert (~emissive[index[hit]] & ~zero_albedo[index[hit]]).sum() >= W * H // 3, "too little of the faceted ring"
    share = float((case.acc[:, 3] == 0).mean())
    assert 0.05 <= share <= 0.2, share
    part = case.reference(iterations=0)["part"]
    rgb = case.acc[part, :3] / case.acc[part, 3:4]
    assert (rgb > 0).all()


@pytest.mark.parametrize("iterations", [0, 1, 5, 8])
@pytest.mark.parametrize("which", list(PARAMS))
@pytest.mark.parametrize("W,H", SIZES)
def test_spatial_restatement_equals_the_reference(world, W, H, which, iterations):
    case = _spatial_case(world, W, H)
    p = dict(iterations=iterations, **PARAMS[which])
    got = denoise_ref.denoise(W, H, world["tris"], case.vis, cs.EYE, case.rg["up"][0], case.acc, **p)
    r = case.compare(f"{W} x {H}, {which}, {iterations} iterations", got, **p)
    cov = case.reference(**p)["coverage"]
    print(f"{r['name']}: error {r['err']:.3g} spread {r['spread']:.3g} tol {r['tol']:.3g} coverage {cov}")
    # the input exercises every edge-stopping term: a tenth of the taps between participating pixels have the term inside
    # (0.05, 0.95). Exempt: the luminance term at 0 iterations (the variance window has none), and the normal term of `other` below
    # 5 iterations: with its (n.n')^8 a 4 degree facet step still weighs 0.98, so that term enters at the wider steps only.
    terms = ["plane"]
    if which == "defaults" or iterations >= 5:
        terms.append("normal")
    if iterations >= 1:
        terms.append("luminance")
    for term in terms:
        assert cov[term] >= 0.1, (term, cov)


def _saved(T):
    return (T.has, T.gx, T.gn, T.hcol, T.hmom, T.rg)


def run_sequence(world, W, H, name, alphas, state_iterations=1, extra=(0, 2)):
    """the restatement over one camera sequence, every call against the reference fed with the restatement's previous state.
    Returns per call: the participating mask, the restatement's h, the figures of the comparisons, and the left-out share."""
    ob, tris, sc = world["ob"], world["tris"], world["sc"]
    ap = dict(alpha_color=alphas[0], alpha_moments=alphas[1])
    T = dtr.TemporalRef(W, H, tris, **ap)
    static = name == "static"
    calls = []
    for k, pose in enumerate(cs.sequence(name, W, H), start=1):
        rg = cs.raygen(ob, pose, W, H)
        vis = sc.raycast(W, H, rg)
        # 96 x 64: the empty records form blocks that stay in place. There the float32 pixel coordinate is 1e-5 px off, and a pixel
        # whose heaviest tap alone is invalid divides that by the little weight that is left (measured: tol 1.9e-4 with scattered
        # empty records, so that input is ill-conditioned for this comparison); 40 x 33 keeps the scattered ones
        acc = cs.accumulation(W, H, 1000 * W + k, empty_seed=7 if (static or W > 40) else None, blocks=W > 40)
        prev, saved = cs.prev_state(T), _saved(T)
        figures = []
        its = tuple(extra) if (not static or k in STATIC_FULL) else ()
        for it in its + (state_iterations,):  # the last one leaves the state for the next call
            T.has, T.gx, T.gn, T.hcol, T.hmom, T.rg = saved
            out, mom = T(vis, pose[0], rg, acc, iterations=it)
            call = cs.TemporalCall(W, H, tris, vis, pose[0], rg, acc, prev, iterations=it, **ap)
            figures += call.compare(f"{name} {W} x {H} {alphas} call {k}, {it} iterations", out, mom, T.hcol)
        calls.append(dict(part=call.part, h=mom[:, 2].copy(), figures=figures, share=call.share, decided=call.r64["decided"]))
    return calls


def _report(calls):
    worst = {}
    for c in calls:
        for f in c["figures"]:
            key = f["name"].split()[-1]
            if key not in worst or f["tol"] > worst[key]["tol"]:
                worst[key] = f
    for key, f in worst.items():
        print(f"{f['name']}: error {f['err']:.3g} spread {f['spread']:.3g} tol {f['tol']:.3g}")
    print(f"left out: at most {max(c['share'] for c in calls):.4%}")


def _decided(calls):
    """over a sequence: the usable taps of weight >= 0.05 that the normal test alone and the plane test alone reject (float64
    reference): both tests must decide taps on their own, or a wrong threshold in one of them could not show"""
    tot = {k: sum(c["decided"][k] for c in calls) for k in ("normal_alone", "plane_alone", "both_pass")}
    print(f"taps decided: {tot}")
    return tot


@pytest.mark.parametrize("name", ["sideways", "dolly"])
@pytest.mark.parametrize("W,H", [(40, 33), (96, 64)])
def test_temporal_translation(world, W, H, name):
    calls = run_sequence(world, W, H, name, (0.2, 0.2))
    _report(calls)
    tot = _decided(calls)
    assert tot["normal_alone"] >= 30 and tot["plane_alone"] >= 100 and tot["both_pass"] >= 1000, tot
    last = calls[-1]
    assert float((last["h"][last["part"]] >= 3).mean()) > 0.7, np.unique(last["h"], return_counts=True)  # the history follows the camera


@pytest.mark.parametrize("W,H", [(40, 33), (96, 64)])
def test_temporal_turn_pushes_a_third_outside(world, W, H):
    calls = run_sequence(world, W, H, "turn", (0.2, 0.2))
    _report(calls)
    tot = _decided(calls)
    assert tot["normal_alone"] >= 10 and tot["plane_alone"] >= 50 and tot["both_pass"] >= 1000, tot
    for c in calls[1:]:
        fresh = float((c["h"][c["part"]] == 1).mean())
        assert 0.25 <= fresh <= 0.5, fresh


@pytest.mark.parametrize("W,H", [(40, 33), (96, 64)])
def test_temporal_half_turn_has_no_history(world, W, H):
    calls = run_sequence(world, W, H, "half_turn", (0.2, 0.2))
    _report(calls)
    for c in calls:
        assert c["part"].sum() > W * H // 2 and (c["h"][c["part"]] == 1).all()


@pytest.mark.parametrize("alphas", [(0.2, 0.2), (0.05, 0.5)])
@pytest.mark.parametrize("W,H", [(40, 33), (96, 64)])
def test_temporal_static_history_grows_to_the_cap(world, W, H, alphas):
    calls = run_sequence(world, W, H, "static", alphas)
    _report(calls)
    assert len(calls) == 36
    for k, c in enumerate(calls, start=1):
        assert (c["h"][c["part"]] == min(k, 32)).all(), k
