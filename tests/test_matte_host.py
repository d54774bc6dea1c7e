"""ID mattes without a GPU: the host build of matte_fold / matte_coverage / matte_pick (platinum_amd/csrc/pt_matte.h through
tests/emu/matte_emu.cpp) against the plain Python restatement of the rule in tests/matte_lib.py, the layout of the three new structs of
include/ptamd.h against platinum_amd/abi.py, the defaults, and the argument checks that need no renderer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_lib as ml  # noqa: E402
from platinum_amd import abi  # noqa: E402

NONE = ml.NONE


def _same(host, ref):
    ref = ml.slots_array(ref)
    assert np.array_equal(host["id"], ref["id"]) and np.array_equal(host["count"], ref["count"]), (host, ref)


def _random_streams(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        distinct = int(rng.integers(1, 41))
        pool = rng.integers(0, 2 ** 32, distinct, dtype=np.uint64).astype(np.uint32)
        # ids 0 and NONE take part like any other
        if rng.random() < 0.5:
            pool[rng.integers(0, distinct)] = 0
        if rng.random() < 0.5:
            pool[rng.integers(0, distinct)] = NONE
        # a skewed draw, so that streams with few and with many distinct ids both occur whatever the pool's size
        w = rng.random(distinct) ** 3
        yield rng.choice(pool, size=int(rng.integers(1, 201)), p=w / w.sum())


def test_fold_equals_the_restatement_on_random_streams():
    over = exact = under = 0
    for ids in _random_streams(10_000, 1):
        _same(ml.host_fold(ids), ml.fold(ids))
        d = np.unique(ids).size
        over += d > ml.SLOTS
        exact += d == ml.SLOTS
        under += d < ml.SLOTS
    assert over > 500 and exact > 100 and under > 500, (over, exact, under)   # every regime of the rule took part


def test_fold_special_streams():
    eight = [7, 0, NONE, 3, 3, 7, 9, 11, 0, 13, 15, 15, NONE]
    assert len(set(eight)) == 8
    ref = ml.fold(eight)
    assert all(c > 0 for _i, c in ref) and sum(c for _i, c in ref) == len(eight)
    _same(ml.host_fold(eight), ref)
    # a ninth distinct id goes to nothing, now and when it comes again; the earlier ones keep counting
    ninth = eight + [99, 7, 99, NONE, 0, 99, 15]
    ref9 = ml.fold(ninth)
    assert [i for i, _c in ref9] == [i for i, _c in ref] and 99 not in [i for i, _c in ref9]
    assert sum(c for _i, c in ref9) == len(ninth) - 3
    _same(ml.host_fold(ninth), ref9)
    # one id only
    one = ml.host_fold([5] * 37)
    _same(one, [(5, 37)] + [(NONE, 0)] * 7)
    # the id of a miss alone: a slot like any other, and not an empty one
    miss = ml.host_fold([NONE] * 3)
    _same(miss, [(NONE, 3)] + [(NONE, 0)] * 7)
    # nothing folded: every slot empty
    _same(ml.host_fold([]), [(NONE, 0)] * 8)


def test_fold_in_chunks_gives_the_same_slots():
    rng = np.random.default_rng(2)
    for ids in _random_streams(500, 3):
        whole = ml.host_fold(ids)
        cuts = np.sort(rng.integers(0, ids.size + 1, int(rng.integers(0, 6))))
        state, ref_state = None, None
        for part in np.split(ids, cuts):           # (empty chunks included)
            state = ml.host_fold(part, state)
            ref_state = ml.fold(part, ref_state)
        assert np.array_equal(state, whole)
        _same(whole, ref_state)


def _slot_images(seed, pixels=400):
    rng = np.random.default_rng(seed)
    slots = np.empty((pixels, ml.SLOTS), ml.SLOT_DTYPE)
    n = np.empty(pixels, np.uint32)
    for p, ids in zip(range(pixels), _random_streams(pixels, seed)):
        ids = ids % np.uint32(24)                  # a small id space: the sets below hit
        if p % 7 == 0:
            ids = np.where(ids == 3, NONE, ids).astype(np.uint32)
        slots[p] = ml.host_fold(ids)
        n[p] = ids.size
    return slots, n, rng


def test_coverage_equals_numpy():
    slots, n, rng = _slot_images(4)
    assert (slots["id"] == NONE).any() and (slots["count"].sum(axis=1) < n).any()
    sets = [[5], [23, 1, 5, 5, 1, 17, 23, 0], list(rng.integers(0, 24, 40)), [NONE], [NONE, 4, NONE], [], [1000], list(range(300))]
    for ids in sets:
        got = ml.host_coverage(slots, ids, n)
        want = ml.coverage(slots, ids, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ids
        assert (got >= 0).all() and (got <= 1).all()
    assert not ml.host_coverage(slots, [], n).any()
    assert not ml.host_coverage(slots, [1000], n).any()
    assert ml.host_coverage(slots, [5], n).any() and ml.host_coverage(slots, [NONE], n).any()
    # every id of a pixel whose ids all fit: coverage exactly 1
    fit = slots["count"].sum(axis=1) == n
    assert fit.any() and (ml.host_coverage(slots, list(range(24)) + [NONE], n)[fit] == 1.0).all()


def test_coverage_of_a_pixel_without_samples_is_zero():
    slots, n, _rng = _slot_images(5, pixels=50)
    zero = np.zeros_like(n)
    assert not ml.host_coverage(slots, list(range(24)), zero).any()           # (slots left over from elsewhere, n = 0)
    empty = np.tile(ml.host_fold([]), (3, 1))
    for k in (0, 5):
        got = ml.host_coverage(empty, [NONE, 0], k)
        assert got.dtype == np.float32 and not got.any() and not np.isnan(got).any()
        assert np.array_equal(got, ml.coverage(empty, [NONE, 0], np.full(3, k, np.uint32)))


def test_pick_takes_the_largest_count_and_the_lowest_slot_among_equals():
    slots, _n, _rng = _slot_images(6, pixels=300)
    ties = 0
    for s in slots:
        k = ml.host_pick(s)
        assert (int(s["id"][k]), int(s["count"][k])) == ml.pick(s)
        assert k == min(j for j in range(ml.SLOTS) if s["count"][j] == s["count"].max())
        ties += int((s["count"] == s["count"].max()).sum() > 1)
    assert ties > 10
    assert ml.host_pick(ml.host_fold([])) == 0


def test_struct_layout_and_constants():
    want = ml.host_layout()
    got = []
    for T in (abi.MatteOptions, abi.MatteSlot, abi.PickResult):
        got += [C.sizeof(T)] + [getattr(T, name).offset for name, _t in T._fields_]
    got += [abi.MATTE_SLOTS, abi.MATTE_NONE, abi.MATTE_INSTANCE, abi.MATTE_MATERIAL]
    assert got == want
    assert C.sizeof(abi.MatteOptions) == 4 and C.sizeof(abi.MatteSlot) == 8 and C.sizeof(abi.PickResult) == 32
    assert np.dtype(abi.MATTE_SLOT_DTYPE) == ml.SLOT_DTYPE and ml.SLOT_DTYPE.itemsize == C.sizeof(abi.MatteSlot)
    assert (ml.SLOTS, ml.NONE, ml.INSTANCE, ml.MATERIAL) == (abi.MATTE_SLOTS, abi.MATTE_NONE, abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def test_defaults(lib):
    o = abi.MatteOptions(enabled=77)
    lib.pt_default_matte_options(C.byref(o))
    assert o.enabled == 0
    lib.pt_default_matte_options(None)      # (a null pointer is ignored, as by the other pt_default_* functions)


def test_argument_checks_that_need_no_renderer(lib):
    INVALID = -1
    o = abi.MatteOptions()
    out = np.zeros(8, np.float32)
    pr = abi.PickResult()
    ids = np.zeros(1, np.uint32)
    assert lib.pt_set_matte_options(None, C.byref(o)) == INVALID
    assert lib.pt_read_matte_slots(None, abi.MATTE_INSTANCE, out.ctypes.data) == INVALID
    assert lib.pt_read_matte(None, abi.MATTE_INSTANCE, ids.ctypes.data, 1, out.ctypes.data) == INVALID
    assert lib.pt_pick(None, 0, 0, C.byref(pr)) == INVALID
    assert b"null" in lib.pt_last_error()
