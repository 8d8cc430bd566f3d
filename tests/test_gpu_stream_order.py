"""Stream ordering under injected delays and on a caller's stream (tests/stream_delay.py has the scripts, the plans and the runner).

rt_wire_delay parks one stream of a context (main, tail or second lane) for a time many times a frame while the others run on; a
consumer on another stream that lacks its event edge then runs before its producer. Every script runs under every plan and stream
mode and must download, bit for bit, what its synchronised reference run downloads (no plan, own stream, rt_sync after every call);
the frame scripts' last checkpoint is also the oracle's frame 12 (10_restir_di.cpp:257-383).

* a. rt_frame back to back in every form of the look-ahead and the tail;  b. the staged API with two lanes;
  c. one call of another kind between unsynchronised frames;
* stream modes: own, a caller's stream, HIP's null stream, switching; the caller-stream modes once more in fresh child processes, one per
  group of scripts and one at a time, with GPU_MAX_HW_QUEUES=8 (`python tests/test_gpu_stream_order.py a|c|strip_c`), where a caller's stream gets a hardware queue of its own;
* rt_wire_delay's error codes, rt_set_stream / rt_get_stream / rt_set_stream_own, rt_destroy with work held on a caller's stream.

The delay is a stimulus, not a threshold: 8 x the measured frame time within [1 ms, 4 ms] (printed), and a run under main_every_gap
must take at least 0.9 x (main holds x delay) of host time, or the GPU's wall-clock rate is not what the library assumes and every
other result of the module is void.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import stream_delay as sd  # noqa: E402

pytestmark = pytest.mark.gpu

FOVY = np.float32(np.pi) / np.float32(4)
RT_OK, RT_ERR_ARG = 0, 1
CALLER_MODES = ("caller", "null", "switching")

_ns, _ref, _oracle = {}, {}, {}


def _api():
    from cedec_2024_rt_amd import api

    return api


def delay_for(script):
    """ns for the script's size, measured once per size: the host time of frame(f); sync() on the undelayed context, the minimum of five"""
    key = (script.W, script.H, script.scene)
    if key not in _ns:
        e = sd.new_context(_api(), script._replace(setup=(), rows=None, halo=0))  # a whole frame of the size, whatever the script runs on
        for f in (1, 2, 3):
            e.r.frame(f)
        e.r.sync()
        best = 1e9
        for f in range(4, 9):
            t0 = time.perf_counter()
            e.r.frame(f)
            e.r.sync()
            best = min(best, time.perf_counter() - t0)
        e.r.close()
        ns = sd.delay_ns(best)
        print(f"stream order: {script.W}x{script.H} {script.scene}: frame {best * 1e6:.0f} us, hold {ns} ns")
        assert ns is not None, f"8 x {best * 1e6:.0f} us is more than {sd.NS_MAX} ns: the image is too large for this test"
        _ns[key] = ns
    return _ns[key]


def reference_of(script):
    if script.name not in _ref:
        _ref[script.name] = sd.reference(_api(), script)
    return _ref[script.name][0]


def uploads_of(script):
    """what the synchronised run uploaded in its upload_* calls: the delayed runs upload the same bytes without a download in front"""
    reference_of(script)
    return _ref[script.name][1]


def _res_bad(a, b, mask):
    return [f for f in a.dtype.names if f != "pad" and not np.array_equal(np.ascontiguousarray(a[f][mask]).view(np.uint8), np.ascontiguousarray(b[f][mask]).view(np.uint8))]


def check_reference_against_oracle(script):
    """the independent reference: the oracle's frame `oracle_frames` is the synchronised run's last checkpoint"""
    from oracle import binding as ob

    key = (script.scene, script.W, script.H, script.oracle_frames, tuple(sorted(script.options.items())))
    if key not in _oracle:
        tris, eye, at = sd._scene(_api(), script.scene)
        ob.lib()
        ob.set_math_mode(ob.MATH_PORTABLE)
        sc = ob.Scene(tris, use_bvh=True)
        rg = ob.raygen_lookat(eye, at, (0, 1, 0), FOVY, script.W, script.H)
        st = ob.new_state(script.W, script.H)
        opt = ob.bench_options(**script.options)
        for f in range(1, script.oracle_frames + 1):
            sc.frame(script.W, script.H, f, rg, np.asarray(eye, np.float32), opt, st, None)
        shaded = (st["vis"]["index"] >= 0) & ~np.isin(st["vis"]["index"], sc.lights)
        _oracle[key] = (st["accum"].copy(), st["pixels"].copy(), st["temporal"].copy(), shaded)
    accum, pixels, temporal, shaded = _oracle[key]
    out = dict((n.split(" ", 2)[2], a) for n, a in reference_of(script)[-3:])
    acc = out["accumulation"]
    nbad = int((acc.view(np.uint32) != accum.reshape(acc.shape).view(np.uint32)).any(axis=1).sum())
    assert nbad == 0, f"{script.name}: frame {script.oracle_frames}: {nbad} pixels of the synchronised run differ from the oracle"
    assert np.array_equal(out["pixels"].reshape(script.H, script.W, 4), pixels), f"{script.name}: pixels differ from the oracle"
    bad = _res_bad(out["RES_TEMPORAL"], temporal.reshape(-1), shaded.reshape(-1))
    assert not bad, f"{script.name}: temporal history differs from the oracle: {bad}"


def check(script, mode, plans=sd.PLANS, oracle=True):
    api = _api()
    ns = delay_for(script)
    want = reference_of(script)
    if script.oracle_frames and oracle:
        check_reference_against_oracle(script)
    for name in plans:
        got = sd.run(api, script, name, mode, ns, uploads=uploads_of(script))
        bad = sd.differences(want, got.out, script.W)
        assert not bad, f"{script.name} under {name} on stream mode {mode} (hold {ns} ns) differs from its synchronised run:\n" + "\n".join(bad)
        if name == "main_every_gap":
            floor = 0.9 * got.main_holds * ns * 1e-9
            print(f"stream order: {script.name} {mode} main_every_gap: {got.main_holds} holds of {ns} ns took {got.seconds * 1e3:.1f} ms (floor {floor * 1e3:.1f} ms)")
            assert got.main_holds == sd.n_gaps(script) and got.seconds >= floor, \
                f"{script.name}: {got.main_holds} main-stream holds of {ns} ns took {got.seconds:.4f} s: the holds did not hold (wall-clock rate?)"


FRAME_SCRIPTS = sd.frame_scripts()
FOREIGN_SCRIPTS = sd.foreign_scripts()


@pytest.mark.parametrize("mode", sd.STREAM_MODES)
@pytest.mark.parametrize("script", FRAME_SCRIPTS, ids=[s.name for s in FRAME_SCRIPTS])
def test_frames_back_to_back(script, mode):
    """a. twelve rt_frames, nothing synchronised but the two checkpoints, under every plan"""
    check(script, mode)


def test_staged_frames_on_two_lanes():
    """b. every stage as the strip driver runs it: upper rows, fork, lower rows on the second lane, end; holds in every gap, the lane's
    wherever rt_lane may be called"""
    script = sd.staged_script()
    assert delay_for(script) * sd.n_gaps(script) * 1e-9 < 0.3  # 193 gaps: holds up to 1.55 ms fit
    check(script, "own")


@pytest.mark.parametrize("mode", sd.STREAM_MODES)
@pytest.mark.parametrize("script", FOREIGN_SCRIPTS, ids=[s.name for s in FOREIGN_SCRIPTS])
def test_foreign_call_between_unsynchronised_frames(script, mode):
    """c. frames 1-3, F, frames 4-6, F, frames 7-8: F and the frames around it do what they do in the synchronised run"""
    check(script, mode)


STRIP_FOREIGN_SCRIPTS = sd.strip_foreign_scripts()


@pytest.mark.parametrize("mode", sd.STREAM_MODES)
@pytest.mark.parametrize("script", STRIP_FOREIGN_SCRIPTS, ids=[s.name for s in STRIP_FOREIGN_SCRIPTS])
def test_halo_call_between_unsynchronised_staged_frames_of_a_strip(script, mode):
    """c on a strip context: rt_halo_pack / _unpack, rt_halo_flags_pack / _unpack and rt_copy_parts between rt_frame_stage frames; the
    reservoir buffers with their halo rows and the device buffers the calls wrote are the synchronised run's"""
    check(script, mode)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_three_local_strips(dense):
    """d. 96x300 in three strips with halo 87 through rt_mg_frame_begin / rt_mg_frame_step, twelve frames, nothing synchronised; every
    rank's main and tail stream held between the sweeps of steps. Every strip's rows == the single context's (and the oracle's)."""
    from cedec_2024_rt_amd.types import bench_options

    api = _api()
    single, sweeps = sd.strips_script(dense)
    W, H = single.W, single.H
    ns = delay_for(single)
    check_reference_against_oracle(single)
    want = dict((n.split(" ", 2)[2], a) for n, a in reference_of(single)[-3:])
    tris, eye, at = sd._scene(api, single.scene)
    bounds = api.mg_partition(H, 3, halo=sd.STRIP_HALO)
    for name in sd.STRIP_PLANS:
        held = sd.plan(name, sweeps)
        ctxs = []
        for b in bounds:
            c = api.Renderer(W, H, rows=b, halo=sd.STRIP_HALO)
            c.set_scene(tris)
            c.lookat(eye, at)
            c.set_options(bench_options())
            c.wire_delay(0, 7, 0)
            c.sync()
            ctxs.append(c)
        hub = api.MgHub(3, renderer=ctxs[0])
        mgs = [api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=hub, flags=api.RT_MG_DENSE if dense else 0) for k, c in enumerate(ctxs)]
        try:
            g = 0
            for f in range(1, sd.FRAMES + 1):
                for m in mgs:
                    m.frame_begin(f)
                live = list(mgs)
                while live:
                    for c in ctxs:
                        for where in ("main", "tail"):
                            if where in held[g % len(held)]:
                                sd.hold(c, where, ns)
                    g += 1
                    live = [m for m in live if m.frame_step()]
            for c, (a, b) in zip(ctxs, bounds):
                lo, hi = (a - c.local_row0) * W, (b - c.local_row0) * W
                got = [(f"rows {a}:{b} {k}", c.download(buf)[lo:hi]) for k, buf in (("accumulation", api.RT_BUF_ACCUMULATION), ("pixels", api.RT_BUF_PIXELS), ("RES_TEMPORAL", api.RT_BUF_RES_TEMPORAL))]
                ref = [(n, want[n.split(" ", 2)[2]][a * W:b * W]) for n, _ in got]
                bad = sd.differences(ref, got, W)
                assert not bad, f"three {'dense' if dense else 'sparse'} strips under {name} (hold {ns} ns) differ from the single context:\n" + "\n".join(bad)
        finally:
            for m in mgs:
                m.close()
            hub.close()
            for c in ctxs:
                c.close()


@pytest.mark.parametrize("group", ["a", "c", "strip_c"])
def test_caller_stream_modes_in_a_fresh_process_with_eight_hardware_queues(group):
    """with the machine's four hardware queues a caller's stream shares one with a stream of the context, and a hold there can stall
    that stream and hide a missing edge; with eight it has one of its own. One child per group of scripts, one at a time, each under a
    time limit of its own."""
    env = dict(os.environ)
    env["GPU_MAX_HW_QUEUES"] = "8"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT)
    out = p.stdout.decode()
    print(out[-4000:])
    assert p.returncode == 0, out[-6000:]
    assert "stream order child: ok" in out


def test_wire_delay_error_codes_leave_the_context_usable():
    api = _api()
    script = sd.frame_scripts()[1]
    want = reference_of(script)
    e = sd.new_context(api, script)
    r = e.r
    L = r.L
    for phase, slot, ns in ((1, 0, 5_000_001), (0, 0, 1 << 40), (0, 8, 0), (1, -1, 1000), (2, 0, 0), (-1, 0, 0)):
        assert L.rt_wire_delay(r.h, phase, slot, ns) == RT_ERR_ARG, (phase, slot, ns)
        assert b"rt_wire_delay" in L.rt_last_error(r.h)
    assert L.rt_wire_delay(r.h, 0, 7, 0) == RT_OK and L.rt_wire_delay(r.h, 1, 7, 5_000_000) == RT_OK  # the borders that are allowed
    for e.step, st in enumerate(script.steps):
        sd.OPS[st.op](e, *st.args)
    r.close()
    assert not sd.differences(want, e.out, script.W)


def test_set_stream_reads_back_and_returns_to_the_own_stream():
    import torch

    api = _api()
    script = sd.frame_scripts()[1]
    want = reference_of(script)
    e = sd.new_context(api, script)
    r = e.r
    own = r.get_stream()
    assert own != 0 and r.side_stream(0) not in (0, own)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (a, b):
        r.set_stream(s.cuda_stream)
        assert r.get_stream() == s.cuda_stream
    r.set_stream(0)
    assert r.get_stream() == 0
    r.set_stream(r.side_stream(0))
    assert r.get_stream() == r.side_stream(0)
    r.set_stream_own()
    assert r.get_stream() == own
    r.lane(True)
    lane = r.get_stream()
    r.lane(False)
    assert lane not in (0, own, r.side_stream(0)) and r.get_stream() == own
    for e.step, st in enumerate(script.steps):
        sd.OPS[st.op](e, *st.args)
    r.close()
    assert not sd.differences(want, e.out, script.W)


def test_destroy_with_work_held_on_a_callers_stream():
    """rt_destroy waits for the caller's stream it was last given, parked or not, and returns"""
    import torch

    api = _api()
    script = sd.frame_scripts()[1]
    ns = delay_for(script)
    e = sd.new_context(api, script)
    s = torch.cuda.Stream()
    e.r.set_stream(s.cuda_stream)
    for f in (1, 2, 3):
        e.r.frame(f)
        for where in sd.STREAMS:
            sd.hold(e.r, where, ns)
    e.r.frame(4)
    e.r.close()
    assert e.r.h is None
    s.synchronize()
    assert not sd.differences(reference_of(script), sd.run(api, script, uploads=uploads_of(script)).out, script.W)  # and the next context is a healthy one


def _child(group):
    """the caller-stream modes of one group of the scripts a and c, every plan (the child of the test above)"""
    import torch

    print("stream order child: GPU_MAX_HW_QUEUES =", os.environ.get("GPU_MAX_HW_QUEUES"), "device", torch.cuda.get_device_name(0))
    t0 = time.perf_counter()
    scripts = dict(a=FRAME_SCRIPTS, c=FOREIGN_SCRIPTS, strip_c=STRIP_FOREIGN_SCRIPTS)[group]
    for script in scripts:
        for mode in CALLER_MODES:
            check(script, mode, oracle=False)  # the parent has held the synchronised runs to the oracle
    print(f"stream order child: ok ({len(scripts)} scripts x {len(CALLER_MODES)} modes x {len(sd.PLANS)} plans in {time.perf_counter() - t0:.1f} s)")


if __name__ == "__main__":
    _child(sys.argv[1])
