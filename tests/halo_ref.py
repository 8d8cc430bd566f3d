"""Plain-numpy statement of the sparse-halo protocol (strips): what the mark, scan, pack and unpack kernels must
produce. Shares no code with csrc/; the set of records a pass touches comes from the oracle's instrumented spatial loop
(oracle.binding.Scene.spatial_reads).

Bitmap buffer of a region of `rows` rows, W pixels wide (uint32 words, rt_halo_bitmap_words): nw = ceil(rows * W / 32),
  word 0             number of set bits,
  words [1, 1+nw)    bit i of word w = pixel 32 w + i of the region, row-major from the region's first row; pad bits 0,
  words [1+nw, 1+2nw) exclusive prefix of the per-word popcounts.
Dense halo bytes of n pixels (rt_halo_pack): n 64-byte records, then n 16-byte radiance records. Sparse list: per set bit, in
bitmap order, the 64-byte record followed by its 16-byte radiance record (80 bytes)."""
import numpy as np

REC, RAD = 64, 16


def n_words(rows, W):
    return (int(rows) * int(W) + 31) // 32


def bitmap_words(rows, W):
    return 1 + 2 * n_words(rows, W)


def _popcount(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.uint64)


def scan(words):
    """words: the 1 + 2 nw words of one bitmap; only the bit words [1, 1+nw) are read. Returns a new array with the count and
    the prefix words rebuilt."""
    words = np.asarray(words, dtype=np.uint32)
    nw = (len(words) - 1) // 2
    assert len(words) == 1 + 2 * nw
    out = words.copy()
    pc = _popcount(words[1:1 + nw])
    cum = np.concatenate([np.zeros(1, np.uint64), np.cumsum(pc, dtype=np.uint64)])
    out[0] = cum[nw]
    out[1 + nw:] = cum[:nw]
    return out


def bits_to_words(bits):
    """bool per pixel of the region -> the 1 + 2 nw words"""
    bits = np.asarray(bits, dtype=bool).ravel()
    nw = (len(bits) + 31) // 32
    padded = np.zeros(nw * 32, dtype=np.uint8)
    padded[:len(bits)] = bits
    out = np.zeros(1 + 2 * nw, dtype=np.uint32)
    out[1:1 + nw] = np.packbits(padded, bitorder="little").view("<u4")
    return scan(out)


def words_to_bits(words, n_pix):
    words = np.asarray(words, dtype=np.uint32)
    nw = (len(words) - 1) // 2
    return np.unpackbits(np.ascontiguousarray(words[1:1 + nw], dtype="<u4").view(np.uint8), bitorder="little")[:n_pix].astype(bool)


def region_bits(picked, W, own_rows, region_row0, region_rows):
    """picked: (pixels of the whole frame, count) buffer indices, -1 = none (touched or read of spatial_reads). The bool per
    region pixel: is it picked by a pixel of rows [own_rows[0], own_rows[1])?"""
    a, b = own_rows
    p = np.asarray(picked)[a * W:b * W].ravel()
    p = p[p >= 0].astype(np.int64)
    lo, hi = region_row0 * W, (region_row0 + region_rows) * W
    p = p[(p >= lo) & (p < hi)] - lo
    bits = np.zeros(region_rows * W, dtype=bool)
    bits[p] = True
    return bits


def need_bitmaps(touched, W, own_rows, region_row0, region_rows):
    """The word array the device must produce for one pass and one side: the bit of every record of the region that a pixel of the
    strip's own rows touches."""
    return bits_to_words(region_bits(touched, W, own_rows, region_row0, region_rows))


def _split(dense_bytes):
    d = np.asarray(dense_bytes, dtype=np.uint8).ravel()
    n = len(d) // (REC + RAD)
    assert len(d) == n * (REC + RAD)
    return d[:n * REC].reshape(n, REC), d[n * REC:].reshape(n, RAD)


def sparse_list(dense_bytes, bits):
    """the 80-byte list entries of the set bits, in bitmap order, as (count * 80) bytes"""
    rec, rad = _split(dense_bytes)
    idx = np.flatnonzero(np.asarray(bits, dtype=bool))
    return np.concatenate([rec[idx], rad[idx]], axis=1).ravel()


def scatter(dense_bytes, bits, lst):
    """dense bytes with the list's entries written over the records of the set bits; every other byte kept"""
    out = np.array(dense_bytes, dtype=np.uint8).ravel()
    rec, rad = _split(out)  # views
    idx = np.flatnonzero(np.asarray(bits, dtype=bool))
    e = np.asarray(lst, dtype=np.uint8).ravel()[:len(idx) * (REC + RAD)].reshape(len(idx), REC + RAD)
    rec[idx] = e[:, :REC]
    rad[idx] = e[:, REC:]
    return out


def patterns(n_pix, seed):
    """the bit contents the scan and the sparse tests run: name -> bool per pixel"""
    rng = np.random.default_rng(seed)
    out = {"zero": np.zeros(n_pix, bool), "ones": np.ones(n_pix, bool)}
    first, last = np.zeros(n_pix, bool), np.zeros(n_pix, bool)
    if n_pix:
        first[0] = True
        last[-1] = True
    out["first"], out["last"] = first, last
    out["d0.03"] = rng.random(n_pix) < 0.03
    out["d0.5"] = rng.random(n_pix) < 0.5
    return out
