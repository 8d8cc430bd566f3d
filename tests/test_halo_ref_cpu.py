"""CPU. The reference of the sparse-halo tests (tests/halo_ref.py, tests/halo_mark_cases.py, the oracle's instrumented spatial
loop) on its own: the instrumented loop is the plain one, its outputs mean what they say, the numpy helpers equal naive loops,
and the chosen cases exercise what tests/test_gpu_halo_kernels.py claims for them."""
import math

import numpy as np
import pytest

import halo_mark_cases as hc
import halo_ref


def _quad_room(oracle, W, H, **optkw):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(scenes.make_quad_room(), use_bvh=True)
    rg = oracle.raygen_lookat(hc.EYE, hc.AT, (0, 1, 0), hc.FOVY, W, H)
    opt, eye = oracle.bench_options(**optkw), np.asarray(hc.EYE, np.float32)
    vis = sc.raycast(W, H, rg)
    r0 = sc.generate_candidate(W, H, 1, vis, eye, opt)
    return sc, vis, opt, eye, r0


def test_halo_ref_instrumented_loop_writes_the_same_bytes_and_counters(oracle):
    W, H = 64, 48
    sc, vis, opt, eye, r0 = _quad_room(oracle, W, H)
    a_in, b_in = r0.copy(), r0.copy()
    a_out, b_out = np.zeros_like(r0), np.zeros_like(r0)
    for pas in range(3):
        ca, cb = oracle.new_counters(), oracle.new_counters()
        sc.spatial_resampling(W, H, 1, pas, vis, eye, opt, a_in, a_out, cnt=ca)
        _, touched, read = sc.spatial_reads(W, H, 1, pas, vis, eye, opt, b_in, b_out, cnt=cb)
        assert a_out.tobytes() == b_out.tobytes(), pas
        assert ca.tobytes() == cb.tobytes(), (pas, ca, cb)
        assert int(ca["spatial_accepted"][0]) > 1000 and (touched >= 0).any() and (read >= 0).any()
        a_in, a_out = a_out, a_in
        b_in, b_out = b_out, b_in


def test_halo_ref_touched_and_read_are_the_loops_own_counts(oracle):
    W, H = 64, 270
    sc, vis, opt, eye, r0 = _quad_room(oracle, W, H)
    cnt = oracle.new_counters()
    _, touched, read = sc.spatial_reads(W, H, 1, 0, vis, eye, opt, r0, cnt=cnt)
    print("accepted", int(cnt["spatial_accepted"][0]), "merged", int(cnt["spatial_merged"][0]))
    assert (touched >= 0).sum() == int(cnt["spatial_accepted"][0]) == 67364
    assert (read >= 0).sum() == int(cnt["spatial_merged"][0]) == 67162
    assert np.array_equal(read[read >= 0], touched[read >= 0])
    assert touched.shape == (W * H, 5) and touched.max() < W * H
    # a neighbour is another pixel, and its row lies within the reach of the largest finite radius of the gaussian
    reach = math.ceil(30.0 / 1.96 * 5.6471)
    pix = np.repeat(np.arange(W * H)[:, None], 5, axis=1)
    on = touched >= 0
    assert (touched[on] != pix[on]).all()
    assert np.abs(touched[on] // W - pix[on] // W).max() <= reach == 87
    # rows restrict the pixels that write, not the neighbours they pick
    _, t2, r2 = sc.spatial_reads(W, H, 1, 0, vis, eye, opt, r0, rows=(90, 180))
    assert np.array_equal(t2[90 * W:180 * W], touched[90 * W:180 * W]) and np.array_equal(r2[90 * W:180 * W], read[90 * W:180 * W])
    assert (t2[:90 * W] == -1).all() and (t2[180 * W:] == -1).all() and (r2[:90 * W] == -1).all() and (r2[180 * W:] == -1).all()


def _naive_scan(words):
    nw = (len(words) - 1) // 2
    out, run = [int(w) for w in words], 0
    for w in range(nw):
        out[1 + nw + w] = run
        run += bin(int(words[1 + w])).count("1")
    out[0] = run
    return out


TINY = [(0, []), (1, [1]), (5, [0, 0, 0, 0, 0]), (32, [1] * 32), (33, [0] * 32 + [1]), (33, [1] + [0] * 31 + [1]), (70, None), (200, None)]


@pytest.mark.parametrize("n_pix,bits", TINY)
def test_halo_ref_helpers_equal_naive_loops(n_pix, bits):
    rng = np.random.default_rng(n_pix)
    bits = np.array(bits, dtype=bool) if bits is not None else rng.random(n_pix) < 0.4
    nw = (n_pix + 31) // 32
    words = halo_ref.bits_to_words(bits)
    assert len(words) == 1 + 2 * nw == halo_ref.bitmap_words(1, n_pix)
    for i in range(nw * 32):  # bit i of word w = pixel 32 w + i; pad bits zero
        assert bool((int(words[1 + i // 32]) >> (i % 32)) & 1) == (bool(bits[i]) if i < n_pix else False)
    assert [int(w) for w in words] == _naive_scan(words)
    garbled = words.copy()
    garbled[0] = 0xFFFFFFFF
    garbled[1 + nw:] = 0xFFFFFFFF
    assert np.array_equal(halo_ref.scan(garbled), words)
    assert np.array_equal(halo_ref.words_to_bits(words, n_pix), bits)
    dense = rng.integers(0, 256, n_pix * 80, dtype=np.uint8)
    lst = halo_ref.sparse_list(dense, bits)
    naive = bytearray()
    for i in range(n_pix):
        if bits[i]:
            naive += dense[i * 64:(i + 1) * 64].tobytes() + dense[n_pix * 64 + i * 16:n_pix * 64 + (i + 1) * 16].tobytes()
    assert lst.tobytes() == bytes(naive) and len(lst) == 80 * int(words[0])
    other = rng.integers(0, 256, n_pix * 80, dtype=np.uint8)
    got = halo_ref.scatter(other, bits, lst)
    want = bytearray(other.tobytes())
    k = 0
    for i in range(n_pix):
        if bits[i]:
            want[i * 64:(i + 1) * 64] = naive[k * 80:k * 80 + 64]
            want[n_pix * 64 + i * 16:n_pix * 64 + (i + 1) * 16] = naive[k * 80 + 64:k * 80 + 80]
            k += 1
    assert got.tobytes() == bytes(want)
    assert halo_ref.scatter(dense, bits, lst).tobytes() == dense.tobytes()


def test_halo_ref_need_bitmaps_places_the_bit_at_region_row_times_w_plus_x():
    W = 37
    touched = np.full((W * 20, 2), -1, np.int32)
    touched[5 * W + 3, 0] = 2 * W + 36    # own row 5 picks (row 2, x 36): region row 0 -> bit 36
    touched[6 * W + 0, 1] = 4 * W + 0     # own row 6 picks (row 4, x 0): region row 2 -> bit 74
    touched[7 * W + 1, 0] = 1 * W + 5     # outside the region's rows
    touched[9 * W + 1, 0] = 3 * W + 5     # not an own row
    words = halo_ref.need_bitmaps(touched, W, (5, 9), 2, 3)
    nw = (3 * W + 31) // 32
    assert len(words) == 1 + 2 * nw and int(words[0]) == 2
    assert [int(w) for w in words[1:1 + nw]] == [0, 1 << 4, 1 << 10, 0]
    assert [int(w) for w in words[1 + nw:]] == [0, 0, 1, 2]


@pytest.mark.parametrize("name", list(hc.CASES))
def test_halo_ref_cases_exercise_what_they_claim(oracle, name):
    ref = hc.reference(oracle, name)
    W, (a, b) = ref.W, ref.rows
    sides = sorted(ref.regions)
    assert sides == {"M3lo": [1], "M3hi": [0]}.get(name, [0, 1])
    n_ref_passes = max(f + n for f, n in ref.calls)
    frames = hc.FRAMES if name in hc.FULL else (1,)
    for frame in frames:
        for pas in range(n_ref_passes):
            assert ref.rows_outside_held("real", frame, pas) == 0
            for side in sides:
                marks = int(ref.bits("real", frame, pas, side).sum())
                print(name, "frame", frame, "pass", pas, "side", side, "marks", marks)
                if name == "M7off":
                    assert marks == 0
                elif frame == 1 or name in hc.FULL:
                    assert marks >= hc.MIN_MARKS[name], (name, frame, pas, side, marks)
    if name in hc.FULL:
        r0, n0 = ref.regions[0]
        r1, n1 = ref.regions[1]
        for frame in frames:
            # the quick reject's rows (40 and more from a side) do mark: beyond 40 rows past the strip's boundary
            far = {0: 0, 1: 0}
            for pas in range(3):
                far[0] += int(ref.bits("real", frame, pas, 0).reshape(n0, W)[:n0 - 40].sum())  # rows < a - 40
                far[1] += int(ref.bits("real", frame, pas, 1).reshape(n1, W)[40:].sum())  # rows >= b + 40
            print(name, "frame", frame, "marks more than 40 rows out", far)
            assert far[0] >= 1 and far[1] >= 1
            for kind, lo, hi in (("random", 0.3, 0.7), ("checker", 0.3, 0.7), ("zero", 1.0, 1.0), ("one", 0.0, 0.0)):
                for pas in range(3):
                    assert ref.rows_outside_held(kind, frame, pas) == 0
                    for side in sides:
                        t, r = ref.bits(kind, frame, pas, side, 0), ref.bits(kind, frame, pas, side, 1)
                        assert not (r & ~t).any()
                        ratio = (t & ~r).sum() / t.sum()
                        print(name, kind, "frame", frame, "pass", pas, "side", side, "marks", int(t.sum()), "unread", round(float(ratio), 3))
                        assert t.sum() >= hc.MIN_MARKS[name] and lo <= ratio <= hi
        # a neighbour's flag decides a draw: the patterns do move the marks
        assert not np.array_equal(ref.bits("zero", 1, 0, 0), ref.bits("one", 1, 0, 0))
    if name == "M4":  # the bands do not meet: own rows in between reach neither region
        t = ref.picks("real", 1, 0)[0][187 * W:213 * W]
        rows = t[t >= 0] // W
        assert ((rows >= a) & (rows < b)).all()
        assert a + ref.halo == 187 and b - ref.halo == 213
    if name == "M5":  # no own row is 40 rows from a side
        assert (b - a) // 2 < 40
