"""CPU: the tile, queue-segment and radiance-buffer index maps (platinum_amd/csrc/pt_layout.h, built for the host by
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
