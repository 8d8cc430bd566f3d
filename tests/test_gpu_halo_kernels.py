"""GPU. The sparse-halo kernels (k_halo_mark<WINDOW>, k_halo_scan / k_halo_scan_sides, k_halo_sparse<PACK>, k_halo_flags<PACK>,
k_shaded_bitmap) against a reference they share no code with: tests/halo_ref.py (numpy) for the scan, the lists and the scatter,
and for the marks the oracle's own spatial loop reporting which records it touches (tests/halo_mark_cases.py). The need-bitmap
of a side and pass must be the `touched` set of the strip's own rows, bit for bit, with its count, prefix and zero pad bits.

Every buffer a call shall write is 0xFF before the call and has guard words on both ends that must stay 0xFF."""
import ctypes as C

import numpy as np
import pytest

import halo_mark_cases as hc
import halo_ref

pytestmark = pytest.mark.gpu
RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, 1, 3  # include/restir_rt.h
G = 64  # guard words (4 bytes each) on each end of a device buffer
FF = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


class Buf:
    """device bytes between two guards; everything 0xFF unless `data` is given"""

    def __init__(self, nbytes, data=None):
        import torch

        assert nbytes % 4 == 0
        host = np.full(2 * G * 4 + nbytes, 0xFF, np.uint8)
        if data is not None:
            host[G * 4:G * 4 + nbytes] = np.asarray(data).view(np.uint8).ravel()
        self.nbytes = nbytes
        self.t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() + G * 4

    def read(self, dtype=np.uint8):
        """the payload; asserts the guards"""
        import torch

        torch.cuda.synchronize()
        host = self.t.cpu().numpy()
        assert (host[:G * 4] == 0xFF).all() and (host[G * 4 + self.nbytes:] == 0xFF).all(), "guard words written"
        return host[G * 4:G * 4 + self.nbytes].copy().view(dtype)


def _bit_words_only(bits):
    """the 1 + 2 nw words as a neighbour receives them: bits valid, count and prefix 0xFF"""
    w = halo_ref.bits_to_words(bits)
    nw = (len(w) - 1) // 2
    w[0] = FF
    w[1 + nw:] = FF
    return w


# ------------------------------------------------------------------------------------------------------------------ a. scan
SCAN = [(32, [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3077]), (37, [1, 7, 28, 887])]


@pytest.mark.parametrize("W,all_rows", SCAN)
def test_halo_scan_equals_the_reference(api, W, all_rows):
    """rt_halo_scan: count and exclusive per-word prefix on both sides of the 256-thread x 4-word step and of the 1024-word chunk
    border, a partial last word (W = 37), an empty bitmap, 1 / 3 / 8 bitmaps per call at stride rt_halo_bitmap_words."""
    ctx = api.Renderer(W, 8)
    names = ["zero", "ones", "first", "last", "d0.03", "d0.5"]
    for n_rows in all_rows:
        words = ctx.halo_bitmap_words(n_rows)
        nw = halo_ref.n_words(n_rows, W)
        assert words == halo_ref.bitmap_words(n_rows, W) == 1 + 2 * nw
        if W == 32:
            assert nw == n_rows
        pats = halo_ref.patterns(n_rows * W, seed=n_rows)
        want_of = {k: halo_ref.bits_to_words(v) for k, v in pats.items()}
        sent_of = {k: _bit_words_only(v) for k, v in pats.items()}
        for n_bitmaps in (1, 3, 8):
            for shift in range(len(names) if n_bitmaps == 1 else 2):
                pick = [names[(3 * shift + i) % len(names)] for i in range(n_bitmaps)] if n_bitmaps > 1 else [names[shift]]
                sent = np.concatenate([sent_of[k] for k in pick])
                want = np.concatenate([want_of[k] for k in pick])
                buf = Buf(4 * len(sent), sent)
                ctx.halo_scan(n_rows, n_bitmaps, buf.ptr)
                ctx.sync()
                got = buf.read(np.uint32)
                for i, k in enumerate(pick):
                    g, w = got[i * words:(i + 1) * words], want[i * words:(i + 1) * words]
                    assert np.array_equal(g[1:1 + nw], w[1:1 + nw]), f"W {W} rows {n_rows} bitmap {i} ({k}): bit words changed"
                    assert int(g[0]) == int(w[0]), f"W {W} rows {n_rows} bitmap {i} ({k}): count {int(g[0])}, reference {int(w[0])}"
                    bad = np.flatnonzero(g[1 + nw:] != w[1 + nw:])
                    assert bad.size == 0, f"W {W} rows {n_rows} bitmap {i} ({k}): prefix differs first at word {bad[0]}: {g[1 + nw + bad[0]]} != {w[1 + nw + bad[0]]}"
    ctx.close()


# ---------------------------------------------------------------------------------------------------- b. sparse pack / unpack
def _sub(dense, n_all, off, n):
    """dense bytes of pixels [off, off + n) out of the dense bytes of n_all pixels"""
    return np.concatenate([dense[off * 64:(off + n) * 64], dense[n_all * 64 + off * 16:n_all * 64 + (off + n) * 16]])


def _put(dense, n_all, off, n, part):
    out = dense.copy()
    out[off * 64:(off + n) * 64] = part[:n * 64]
    out[n_all * 64 + off * 16:n_all * 64 + (off + n) * 16] = part[n * 64:]
    return out


def _scanned(ctx, n_rows, bits):
    """device bitmap of `bits` with count and prefix from rt_halo_scan, checked against the reference"""
    bm = Buf(4 * ctx.halo_bitmap_words(n_rows), _bit_words_only(bits))
    ctx.halo_scan(n_rows, 1, bm.ptr)
    ctx.sync()
    assert np.array_equal(bm.read(np.uint32), halo_ref.bits_to_words(bits))
    return bm


SPARSE = [(37, 64, [(0, 64), (5, 1), (63, 1)]), (200, 200, [(0, 200)])]


@pytest.mark.parametrize("W,H,ranges", SPARSE)
def test_halo_sparse_pack_and_unpack_equal_the_reference(api, W, H, ranges):
    """rt_halo_pack_sparse: the list is the marked records in bitmap order, nothing behind it is written. rt_halo_unpack_sparse:
    the marked records take the list's bytes, every other record of the context keeps every byte. 200 x 200: nw = 1250, list
    indices of the upper part come from the scan's second chunk."""
    ctx = api.Renderer(W, H)
    res, n_all = api.RT_RES_0, W * H
    rng = np.random.default_rng(W)
    A = rng.integers(0, 256, n_all * 80, dtype=np.uint8)  # arbitrary bytes, NaN patterns included
    B = rng.integers(0, 256, n_all * 80, dtype=np.uint8)
    dA, dB = Buf(len(A), A), Buf(len(B), B)
    assert ctx.halo_bytes(H) == n_all * 80
    for row0, n_rows in ranges:
        off, n = row0 * W, n_rows * W
        for name, bits in halo_ref.patterns(n, seed=row0 + n_rows).items():
            count = int(bits.sum())
            bm = _scanned(ctx, n_rows, bits)
            # pack
            ctx.halo_unpack(res, 0, H, dA.ptr)
            lst = Buf(80 * n)
            ctx.halo_pack_sparse(res, row0, n_rows, bm.ptr, lst.ptr)
            ctx.sync()
            got = lst.read()
            want = halo_ref.sparse_list(_sub(A, n_all, off, n), bits)
            assert len(want) == 80 * count
            assert np.array_equal(got[:80 * count], want), f"{W}x{H} rows {row0}+{n_rows} {name}: list differs"
            assert (got[80 * count:] == 0xFF).all(), f"{W}x{H} rows {row0}+{n_rows} {name}: bytes behind the list written"
            # unpack
            ctx.halo_unpack(res, 0, H, dB.ptr)
            src = Buf(80 * n, np.concatenate([want, np.full(80 * (n - count), 0xFF, np.uint8)]))
            ctx.halo_unpack_sparse(res, row0, n_rows, bm.ptr, src.ptr)
            back = Buf(80 * n_all)
            ctx.halo_pack(res, 0, H, back.ptr)
            ctx.sync()
            expect = _put(B, n_all, off, n, halo_ref.scatter(_sub(B, n_all, off, n), bits, want))
            g = back.read()
            assert np.array_equal(g, expect), f"{W}x{H} rows {row0}+{n_rows} {name}: {int((g != expect).sum())} bytes differ after the unpack"
            unmarked = np.concatenate([np.repeat(~np.pad(bits, (off, n_all - off - n)), 64), np.repeat(~np.pad(bits, (off, n_all - off - n)), 16)])
            assert np.array_equal(g[unmarked], B[unmarked])
    ctx.close()


def test_halo_sparse_two_ranges_equal_two_single_calls(api):
    """rt_halo_{pack,unpack}_sparse_ranges with ranges of unequal size (the grid is sized by the larger), in both orders"""
    W, H = 37, 64
    ctx = api.Renderer(W, H)
    L, res, n_all = ctx.L, api.RT_RES_0, W * H
    rng = np.random.default_rng(5)
    A = rng.integers(0, 256, n_all * 80, dtype=np.uint8)
    B = rng.integers(0, 256, n_all * 80, dtype=np.uint8)
    dA, dB = Buf(len(A), A), Buf(len(B), B)
    big, small = (2, 30), (50, 3)
    bits = {big: rng.random(30 * W) < 0.5, small: rng.random(3 * W) < 0.3}
    bms = {r: _scanned(ctx, r[1], bits[r]) for r in (big, small)}
    want = {r: halo_ref.sparse_list(_sub(A, n_all, r[0] * W, r[1] * W), bits[r]) for r in (big, small)}
    assert all(0 < len(want[r]) < 80 * r[1] * W for r in want)

    def arrays(order, bufs):
        return ((C.c_int * 2)(*[r[0] for r in order]), (C.c_int * 2)(*[r[1] for r in order]),
                (C.c_void_p * 2)(*[bms[r].ptr for r in order]), (C.c_void_p * 2)(*[bufs[r].ptr for r in order]))

    single = {}
    ctx.halo_unpack(res, 0, H, dA.ptr)
    for r in (big, small):
        lst = Buf(80 * r[1] * W)
        ctx.halo_pack_sparse(res, r[0], r[1], bms[r].ptr, lst.ptr)
        ctx.sync()
        single[r] = lst.read()
    for order in ((big, small), (small, big)):
        lists = {r: Buf(80 * r[1] * W) for r in order}
        row0, n_rows, bm, dst = arrays(order, lists)
        assert L.rt_halo_pack_sparse_ranges(ctx.h, res, 2, row0, n_rows, bm, dst) == RT_OK
        ctx.sync()
        for r in order:
            got = lists[r].read()
            assert np.array_equal(got, single[r]), (order, r)
            assert np.array_equal(got[:len(want[r])], want[r]) and (got[len(want[r]):] == 0xFF).all(), (order, r)
    # unpack: both ranges in one call, each order, against two single calls and the reference
    expect = B
    for r in (big, small):
        expect = _put(expect, n_all, r[0] * W, r[1] * W, halo_ref.scatter(_sub(B, n_all, r[0] * W, r[1] * W), bits[r], want[r]))
    srcs = {r: Buf(80 * r[1] * W, np.concatenate([want[r], np.full(80 * r[1] * W - len(want[r]), 0xFF, np.uint8)])) for r in (big, small)}
    results = []
    for order in (None, (big, small), (small, big)):
        ctx.halo_unpack(res, 0, H, dB.ptr)
        if order is None:
            for r in (big, small):
                ctx.halo_unpack_sparse(res, r[0], r[1], bms[r].ptr, srcs[r].ptr)
        else:
            row0, n_rows, bm, src = arrays(order, srcs)
            assert L.rt_halo_unpack_sparse_ranges(ctx.h, res, 2, row0, n_rows, bm, src) == RT_OK
        back = Buf(80 * n_all)
        ctx.halo_pack(res, 0, H, back.ptr)
        ctx.sync()
        results.append(back.read())
    for g in results:
        assert np.array_equal(g, expect), int((g != expect).sum())
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ c. marks
def _strip(api, ref):
    from cedec_2024_rt_amd.types import bench_options

    ctx = api.Renderer(ref.W, ref.H, rows=ref.rows, halo=ref.halo)
    ctx.set_scene(ref.tris)
    ctx.lookat(hc.EYE, hc.AT)
    ctx.set_options(bench_options(**ref.optkw))
    assert ctx.raygen().tobytes() == ref.rg.tobytes()
    got = ctx.options()
    assert all(np.array_equal(got[f], ref.opt[f]) for f in ref.opt.dtype.names)
    assert (ctx.local_row0, ctx.local_row0 + ctx.local_rows) == ref.held
    ctx.raycast()
    ctx.sync()
    return ctx


def _set_flags(ctx, ref, kind):
    for side, f in ref.flags(kind).items():
        r0, n = ref.regions[side]
        assert ctx.halo_flags_bytes(n) == len(f)
        b = Buf((len(f) + 3) // 4 * 4, np.concatenate([f, np.zeros(-len(f) % 4, np.uint8)]))
        ctx.halo_flags_unpack(r0, n, b.ptr)
        ctx.sync()


def _mark(ctx, ref, frame, first, n_passes, layout="apart", sides=None):
    """rt_halo_mark_sides into 0xFF buffers; side -> words. layout "apart": side 1 lies in front of side 0 with guard words in
    between (two clears); "together": side 0 then side 1 back to back in one allocation (the single clear)."""
    import torch

    sides = sorted(ref.regions) if sides is None else sides
    words = {s: ctx.halo_bitmap_words(ref.regions[s][1]) for s in sides}
    for s in sides:
        assert words[s] == halo_ref.bitmap_words(ref.regions[s][1], ref.W)
    order = sorted(sides, reverse=(layout == "apart"))
    gap = G if layout == "apart" else 0
    off, pos = {}, G
    for s in order:
        off[s] = pos
        pos += n_passes * words[s] + gap
    total = pos + (G - gap)
    t = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = {s: C.c_void_p(t.data_ptr() + 4 * off[s]) for s in sides}
    rc = ctx.L.rt_halo_mark_sides(ctx.h, frame, first, n_passes, ptr.get(0), ptr.get(1))
    assert rc == RT_OK, ctx.L.rt_last_error(ctx.h).decode()
    ctx.sync()
    host = t.cpu().numpy().view(np.uint32)
    inside = np.zeros(total, bool)
    out = {}
    for s in sides:
        inside[off[s]:off[s] + n_passes * words[s]] = True
        out[s] = host[off[s]:off[s] + n_passes * words[s]].copy()
    assert (host[~inside] == FF).all(), "guard words written"
    return out


def _check(got, want, what):
    assert sorted(got) == sorted(want), what
    for s in got:
        if not np.array_equal(got[s], want[s]):
            nb = len(want[s])
            bad = np.flatnonzero(got[s] != want[s])
            raise AssertionError(f"{what}, side {s}: {bad.size} of {nb} words differ, first at word {bad[0]}: device {got[s][bad[0]]:#x}, reference "
                                 f"{want[s][bad[0]]:#x}; counts device {int(got[s][0])}, reference {int(want[s][0])}")


def _tunings(api):
    keys = (api.Tune.MARK_QUICK, api.Tune.MARK_WINDOW, api.Tune.MARK_SPLIT, api.Tune.MARK_CACHE)
    return keys, [tuple((i >> b) & 1 for b in range(4)) for i in range(16)]


FAR_EYE = (0.5, 2.5, 12.0)  # from here the frame holds sky beside the room; the cases' camera sees walls and lights only


@pytest.mark.parametrize("W,H", sorted({(c[0], c[1]) for c in hc.CASES.values()}))
def test_halo_flags_pack_gives_the_oracles_flags(api, oracle, W, H):
    """k_halo_flags<PACK> and the G-buffer's flag word: 1 on a shaded pixel, 2 on an emissive one, 0 on sky, as the oracle's raycast
    says; single rows in the middle of the frame too."""
    name = next(k for k, c in hc.CASES.items() if (c[0], c[1]) == (W, H))
    ref = hc.reference(oracle, name)
    ctx = api.Renderer(W, H)
    ctx.set_scene(ref.tris)
    ctx.set_options(ref.opt)
    for eye, values in ((hc.EYE, {1, 2}), (FAR_EYE, {0, 1, 2})):
        if eye == hc.EYE:
            want = ref.real
        else:
            rg = oracle.raygen_lookat(eye, hc.AT, (0, 1, 0), hc.FOVY, W, H)
            want = hc.flag_bytes(oracle, ref.sc, ref.sc.raycast(W, H, rg))
        assert set(np.unique(want).tolist()) == values
        ctx.lookat(eye, hc.AT)
        ctx.raycast()
        for row0, n in ((0, H), (H // 3, 1), (H - 2, 2)):
            nb = ctx.halo_flags_bytes(n)
            assert nb == n * W
            b = Buf((nb + 3) // 4 * 4)
            ctx.halo_flags_pack(row0, n, b.ptr)
            ctx.sync()
            got = b.read()
            assert np.array_equal(got[:nb], want[row0 * W:(row0 + n) * W]), f"eye {eye}: {int((got[:nb] != want[row0 * W:(row0 + n) * W]).sum())} flags differ"
            assert (got[nb:] == 0xFF).all()
    ctx.close()


@pytest.mark.parametrize("name", list(hc.CASES))
def test_halo_marks_equal_the_touched_set_of_the_oracles_loop(api, oracle, name):
    """rt_halo_mark_sides / rt_halo_mark: the whole word array (count, bits, prefix, zero pad bits) of every pass and side equals
    halo_ref.need_bitmaps of the records the oracle's spatial loop touches from the strip's own rows."""
    ref = hc.reference(oracle, name)
    ctx = _strip(api, ref)
    keys, settings = _tunings(api)
    default = tuple(ctx.tuning_get(k) for k in keys)
    assert default == (1, 1, 0, 1)
    sides = sorted(ref.regions)
    full = name in hc.FULL

    # errors first: flags into own rows, a mark on a side without neighbour
    a, b = ref.rows
    junk = Buf(4 * ((ref.W + 3) // 4))
    assert ctx.L.rt_halo_flags_unpack(ctx.h, a, 1, C.c_void_p(junk.ptr)) == RT_ERR_ARG
    assert ctx.L.rt_halo_flags_unpack(ctx.h, b - 1, 1, C.c_void_p(junk.ptr)) == RT_ERR_ARG
    for side in (0, 1):
        if side not in ref.regions:
            bm = Buf(4 * 3 * halo_ref.bitmap_words(ref.halo, ref.W))
            assert ctx.L.rt_halo_mark(ctx.h, 1, 0, 3, side, C.c_void_p(bm.ptr)) == RT_ERR_STATE
            assert (bm.read() == 0xFF).all()

    kinds = hc.FLAG_KINDS if full else ("real",)
    frames = hc.FRAMES if full else (1,)
    for kind in kinds:  # a new pattern on the live context: the cached bit rows must follow it (Tune.MARK_CACHE)
        _set_flags(ctx, ref, kind)
        for frame in frames:
            for first, n in ref.calls:
                _check(_mark(ctx, ref, frame, first, n), ref.expected(kind, frame, first, n), f"{name} {kind} flags frame {frame} passes {first}+{n}")
    # both sides in one allocation (one clear over both) and the single-side entry point
    for kind in (("random", "real") if full else ("real",)):
        _set_flags(ctx, ref, kind)
        first, n = ref.calls[0]
        want = ref.expected(kind, 1, first, n)
        _check(_mark(ctx, ref, 1, first, n, layout="together"), want, f"{name} {kind} flags, one allocation")
        for s in sides:
            words = ctx.halo_bitmap_words(ref.regions[s][1])
            bm = Buf(4 * n * words)
            ctx.halo_mark(1, first, n, s, bm.ptr)
            ctx.sync()
            _check({s: bm.read(np.uint32)}, {s: want[s]}, f"{name} {kind} flags, rt_halo_mark side {s}")
        # every form of the kernel (the flags are `kind`'s from here on; "real" last)
        for setting in (settings if full else [(0, 0, 0, 0)]):
            for k, v in zip(keys, setting):
                ctx.tuning(k, v)
            for frame in frames:
                for first, n in ref.calls:
                    _check(_mark(ctx, ref, frame, first, n), ref.expected(kind, frame, first, n),
                           f"{name} {kind} flags frame {frame} passes {first}+{n} tuning quick/window/split/cache {setting}")
        for k, v in zip(keys, default):
            ctx.tuning(k, v)
    if name == "M7off":
        got = _mark(ctx, ref, 1, 0, 3)
        assert all((g == 0).all() for g in got.values())
    ctx.close()
