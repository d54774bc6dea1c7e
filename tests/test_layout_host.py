"""CPU: the tile, queue-segment and radiance-buffer index maps (platinum_amd/csrc/pt_layout.h; the tile folds' fold_tile and fold_stage of
pt_tilefold.h; built for the host by
tests/emu/layout_probe.cpp, a part of the host harness of tests/host_build.py) against the properties every kernel relies on, enumerated exhaustively over small queue plans
(platinum_amd/csrc/queue_plan.h plan_queues): images with partial tiles on both edges, sample counts that are no multiple of the
eight-sample staging round, one and several tiles per segment, one and several bands."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import host_build


class Plan(C.Structure):  # include/ptamd.h pt_queue_plan
    _fields_ = [("samples_in_flight", C.c_uint32), ("tiles_per_seg", C.c_uint32), ("nseg", C.c_uint32), ("seg_cap", C.c_uint32),
                ("capacity", C.c_uint64), ("lbuf_entries", C.c_uint64)]


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load()
    L.lp_plan.argtypes = [C.c_uint32] * 5 + [C.POINTER(Plan)]
    L.lp_tile_count.argtypes = [C.c_uint32] * 2
    L.lp_tile_count.restype = C.c_uint32
    L.lp_meta_pid_bits.restype = C.c_uint32
    L.lp_seg_queue_slots.argtypes = [C.c_uint32] * 2
    L.lp_seg_queue_slots.restype = C.c_uint64
    L.lp_slots.argtypes = [C.c_uint32] * 2 + [C.c_void_p] * 2
    L.lp_segments.argtypes = [C.c_uint32] * 4 + [C.c_void_p] * 2
    L.lp_lbuf.argtypes = [C.c_uint32] * 2 + [C.c_void_p]
    L.lp_pixels.argtypes = [C.c_uint32] * 2 + [C.c_void_p] * 4
    L.lp_tile_pixels.argtypes = [C.c_uint32] * 2 + [C.c_void_p]
    L.lp_fold_tiles.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 4
    L.lp_fold_stage.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    L.lp_fold_stage.restype = C.c_uint32
    L.lp_fold_row.restype = C.c_uint32
    return L


def _u32(n):
    return np.zeros(n, np.uint32)


SIZES = [(33, 17), (8, 40)]
PLANS = list(itertools.product(SIZES, [1, 3, 8, 9], [0, 3], [1, 4]))


@pytest.mark.parametrize("size,nsamples,tps_override,bands", PLANS)
def test_segments_and_radiance_buffer(size, nsamples, tps_override, bands):
    L = lib()
    W, H = size
    plan = Plan()
    assert L.lp_plan(W, H, nsamples, tps_override, bands, C.byref(plan)) == 0
    tiles = L.lp_tile_count(W, H)
    assert tiles == ((W + 7) // 8) * ((H + 7) // 8)
    nseg, cap, tps = plan.nseg, plan.seg_cap, plan.tiles_per_seg
    assert plan.samples_in_flight == nsamples and cap == tps * nsamples * 64 and nseg % bands == 0
    assert plan.lbuf_entries == tiles * 64 * nsamples
    assert plan.capacity == L.lp_seg_queue_slots(nseg, cap)

    # seg_slot: injective over (sg < nseg, r < seg_cap), inside the queue arrays, inverted by slot_segment
    slot, owner = _u32(nseg * cap), _u32(nseg * cap)
    L.lp_slots(nseg, cap, slot.ctypes.data, owner.ctypes.data)
    assert np.unique(slot).size == slot.size
    assert int(slot.max()) < plan.capacity
    assert np.array_equal(owner, np.repeat(np.arange(nseg, dtype=np.uint32), cap))

    # segments: sg -> first tile / tiles_per_seg is a permutation of [0, nseg); the tile ranges cover [0, tiles)
    first, base = _u32(nseg), _u32(nseg)
    L.lp_segments(nseg, bands, tps, nsamples, first.ctypes.data, base.ctypes.data)
    assert np.array_equal(first % tps, np.zeros(nseg, np.uint32))
    assert np.array_equal(np.sort(first // tps), np.arange(nseg, dtype=np.uint32))
    covered = np.zeros(nseg * tps, bool)
    for f in first:
        covered[f:f + tps] = True
    assert covered[:tiles].all()
    assert np.array_equal(base, first * nsamples * 64)

    # lbuf_index: a bijection of (tile, lane, s) onto [0, tiles * 64 * nsamples); relative to its segment's window every entry fits in
    # seg_cap, hence in the bits of rayD.w that carry it
    idx = _u32(tiles * 64 * nsamples)
    L.lp_lbuf(tiles, nsamples, idx.ctypes.data)
    assert np.array_equal(np.sort(idx), np.arange(idx.size, dtype=np.uint32))
    seg_of_index = np.empty(nseg, np.int64)   # first // tps -> sg
    seg_of_index[first // tps] = np.arange(nseg)
    tile_of_entry = np.repeat(np.arange(tiles), 64 * nsamples)
    rel = idx.astype(np.int64) - base[seg_of_index[tile_of_entry // tps]].astype(np.int64)
    assert rel.min() >= 0 and rel.max() < cap
    assert L.lp_meta_pid_bits() == 21 and cap <= 1 << 21


@pytest.mark.parametrize("size", SIZES)
def test_tiles_and_pixels(size):
    L = lib()
    W, H = size
    tiles = L.lp_tile_count(W, H)
    tile, lane, pid1, back = _u32(W * H), _u32(W * H), _u32(W * H), _u32(W * H)
    L.lp_pixels(W, H, tile.ctypes.data, lane.ctypes.data, pid1.ctypes.data, back.ctypes.data)
    xy = _u32(tiles * 64 * 2)
    L.lp_tile_pixels(W, H, xy.ctypes.data)
    xy = xy.reshape(tiles, 64, 2)
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    assert int(tile.max()) < tiles and int(lane.max()) < 64
    # tile_pixel(tile_of_pixel, lane_of_pixel) == (x, y) for every pixel
    assert np.array_equal(xy[tile, lane, 0], xs) and np.array_equal(xy[tile, lane, 1], ys)
    # every other (tile, lane) is a lane of a partial tile and maps outside the image
    inside = np.zeros((tiles, 64), bool)
    inside[tile, lane] = True
    assert inside.sum() == W * H
    out = ~inside
    assert out.sum() == tiles * 64 - W * H
    assert ((xy[..., 0] >= W) | (xy[..., 1] >= H))[out].all()
    assert ((xy[..., 0] < W) & (xy[..., 1] < H))[inside].all()
    # the one-sample pid -> pixel map inverts lbuf_index(..., nsamples = 1)
    assert np.array_equal(pid1, tile * 64 + lane)
    assert np.array_equal(back, np.arange(W * H, dtype=np.uint32))


FOLD_SIZES = [(1, 1), (8, 8), (17, 9), (64, 40)]


def _fold_tiles(W, H, ntiles, active=None, count=None, rect=None):
    """fold_tile of every (tile < ntiles, lane): itile, live, inside, x, y as (ntiles, 64) arrays."""
    out = _u32(ntiles * 64 * 5)
    a = None if active is None else np.ascontiguousarray(active, np.uint32)
    c = None if count is None else np.array([count], np.uint32)
    r = None if rect is None else np.array(rect, np.uint32)
    lib().lp_fold_tiles(W, H, ntiles, None if a is None else a.ctypes.data, None if c is None else c.ctypes.data,
                        None if r is None else r.ctypes.data, out.ctypes.data)
    out = out.reshape(ntiles, 64, 5)
    return out[..., 0], out[..., 1].astype(bool), out[..., 2].astype(bool), out[..., 3], out[..., 4]


def _tile_xy(itile, W):
    """numpy restatement: pixel of (image tile, lane), lanes row-major in the 8x8 tile, tiles row-major in the image."""
    tx = (W + 7) // 8
    lane = np.arange(64, dtype=np.int64)[None, :]
    it = itile.astype(np.int64)
    return (it % tx) * 8 + lane % 8, (it // tx) * 8 + lane // 8


@pytest.mark.parametrize("size", FOLD_SIZES)
def test_fold_tile_full_frame(size):
    W, H = size
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    extra = 3   # tile indices at and beyond the tile count (the last block of k_accumulate is padded to four waves): not live
    itile, live, inside, x, y = _fold_tiles(W, H, tiles + extra)
    assert np.array_equal(itile, np.repeat(np.arange(tiles + extra, dtype=np.uint32)[:, None], 64, 1))
    assert live[:tiles].all() and not live[tiles:].any() and not inside[tiles:].any()
    ex, ey = _tile_xy(itile[:tiles], W)
    assert np.array_equal(x[:tiles], ex) and np.array_equal(y[:tiles], ey)
    assert np.array_equal(inside[:tiles], (ex < W) & (ey < H))
    # every pixel of the image is inside exactly once
    hits = np.zeros((H, W), np.int64)
    np.add.at(hits, (y[inside], x[inside]), 1)
    assert (hits == 1).all()


@pytest.mark.parametrize("size", FOLD_SIZES)
def test_fold_tile_virtual_tiles(size):
    W, H = size
    tx, ty = (W + 7) // 8, (H + 7) // 8
    # a rectangle that cuts through tiles on all four sides where the image is large enough for one
    rect = (3, 2, W - 2, H - 3) if W > 5 and H > 5 else (0, 0, W, H)
    active = np.arange(tx * ty, dtype=np.uint32)[::2] if tx * ty > 2 else np.arange(tx * ty, dtype=np.uint32)   # ascending, not contiguous
    capacity = active.size
    for count in sorted({capacity, max(capacity - 1, 0)}):
        # tile indices at and beyond the count (the grid is sized for the first list): not live, whatever the list holds there
        itile, live, inside, x, y = _fold_tiles(W, H, capacity + 2, np.concatenate([active, [0, 0]]), count, rect)
        assert live[:count].all() and not live[count:].any() and not inside[count:].any()
        assert np.array_equal(itile[:count], np.repeat(active[:count, None], 64, 1)) and not itile[count:].any()
        ex, ey = _tile_xy(itile[:count], W)
        assert np.array_equal(x[:count], ex) and np.array_equal(y[:count], ey)
        assert np.array_equal(inside[:count], (ex >= rect[0]) & (ex < rect[2]) & (ey >= rect[1]) & (ey < rect[3]))
        # the pixels folded: those of the rectangle that lie in a listed tile, once each
        hits = np.zeros((H, W), np.int64)
        np.add.at(hits, (y[inside], x[inside]), 1)
        ys, xs = np.mgrid[0:H, 0:W]
        listed = np.isin((ys // 8) * tx + xs // 8, active[:count])
        want = listed & (xs >= rect[0]) & (xs < rect[2]) & (ys >= rect[1]) & (ys < rect[3])
        assert np.array_equal(hits, want.astype(np.int64))


@pytest.mark.parametrize("nsamples", [1, 7, 8, 9, 64])
def test_fold_stage_sequence(nsamples):
    L = lib()
    assert L.lp_fold_row() == 9
    tile = 5
    want = _u32(6 * 64 * nsamples)
    L.lp_lbuf(6, nsamples, want.ctypes.data)   # lbuf_index in (tile, lane, s) enumeration order
    want = want.reshape(6, 64, nsamples)[tile]
    seen = np.zeros((64, nsamples), np.int64)
    for s0 in range(0, nsamples, 8):
        nb = min(8, nsamples - s0)
        out = _u32(2 * 512)
        n = L.lp_fold_stage(tile, s0, nb, nsamples, out.ctypes.data)
        assert n == 64 * nb
        pid, slot = out[:2 * n:2], out[1:2 * n:2]
        px, j = slot // 9, slot % 9
        assert int(px.max()) < 64 and int(j.max()) < nb
        assert np.unique(slot).size == n   # no two loads of a round share an LDS slot
        s = s0 + j
        assert np.array_equal(slot, px * 9 + (s % 8))
        assert np.array_equal(pid, want[px, s])
        np.add.at(seen, (px, s), 1)
    assert (seen == 1).all()   # over the rounds every (pixel, sample) is staged exactly once
