"""Host side of the ID-matte tests: a plain Python restatement of the fold (dict + list), of the resolve and of the pick; the
independent reference of the GPU tests, the oracle's trace_primary(s) for s = 0 .. n - 1 folded by that restatement, with the material id
taken from the scene's own material_slots and the prefix sum of its instances' material counts; and the ctypes wrapper of
tests/emu/matte_emu.cpp (the host build of platinum_amd/csrc/pt_matte.h, a library of its own).  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import host_build  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "matte_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_matte.so")
SLOTS = 8
NONE = 0xFFFFFFFF
INSTANCE, MATERIAL = 0, 1
SLOT_DTYPE = np.dtype([("id", "<u4"), ("count", "<u4")])


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def fold(ids, state=None):
    """The slots after folding `ids` in order: a list of SLOTS (id, count), first come, no eviction; `state` = the slots before."""
    state = [(int(i), int(c)) for i, c in (state if state is not None else [])]
    order = [i for i, c in state if c]                  # the occupied slots' ids, in slot order
    count = {i: c for i, c in state if c}
    for x in ids:
        x = int(x)
        if x in count:
            count[x] += 1
        elif len(order) < SLOTS:
            order.append(x)
            count[x] = 1
    return [(i, count[i]) for i in order] + [(NONE, 0)] * (SLOTS - len(order))


def slots_array(slot_list):
    return np.array(slot_list, dtype=np.uint32).view(SLOT_DTYPE).reshape(SLOTS)


def fold_image(ids, counts=None):
    """ids: (n, H, W) uint32, sample-major.  (H, W, SLOTS) slots of every pixel after its first counts[y, x] samples (default: all n)."""
    n, H, W = ids.shape
    out = np.empty((H, W, SLOTS), SLOT_DTYPE)
    for y in range(H):
        for x in range(W):
            out[y, x] = slots_array(fold(ids[: n if counts is None else int(counts[y, x]), y, x]))
    return out


def coverage(slots, ids, n):
    """numpy's resolve: float32(sum of the counts of the slots whose id is in `ids`) / float32(n), 0 where n = 0.  slots (..., SLOTS), n (...)."""
    member = np.isin(slots["id"], np.asarray(list(ids), np.uint32))
    total = np.where(member, slots["count"], 0).sum(axis=-1, dtype=np.uint64)
    n = np.broadcast_to(np.asarray(n, np.uint32), total.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = total.astype(np.float32) / n.astype(np.float32)
    return np.where(n == 0, np.float32(0), q).astype(np.float32)


def pick(slots):
    """(id, count) of the slot with the largest count, ties to the lowest slot.  slots (SLOTS,)."""
    k = int(np.argmax(slots["count"]))      # (numpy's argmax returns the first of equals)
    return int(slots["id"][k]), int(slots["count"][k])


def distinct_ids(ids):
    """(H, W) number of distinct values along axis 0 of an (n, H, W) id volume."""
    s = np.sort(ids, axis=0)
    return 1 + (s[1:] != s[:-1]).sum(axis=0)


# ---- the reference: the oracle's camera rays ------------------------------------------------------------------------------------------------
def material_bases(scene):
    """[instance] index of its first material in the flattened table: the prefix sum of the instances' material counts."""
    counts = [len(node.materials) for node in scene.nodes]
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)


def reference_ids(scene, size, spp, first_sample=0):
    """(instance ids, material ids), each (spp, H, W) uint32 with NONE for a miss: the oracle's trace_primary, sample by sample."""
    import oracle_lib
    from platinum_amd.renderer import make_params
    W, H = size
    o = oracle_lib.OracleScene(scene, make_params(W, H, spp, 4, first_sample=first_sample))
    base = material_bases(scene)
    mesh_of = np.array([node.mesh for node in scene.nodes], np.int64)
    slot_tables = [np.asarray(m.material_slots, np.uint32) for m in scene.meshes]
    inst = np.empty((spp, H, W), np.uint32)
    mat = np.empty((spp, H, W), np.uint32)
    try:
        for s in range(spp):
            rec = o.trace_primary(first_sample + s)
            i, prim = rec["instance"].astype(np.int64), rec["primitive"].astype(np.int64)
            hit = i >= 0
            m = np.full((H, W), NONE, np.uint32)
            for mesh in np.unique(mesh_of[i[hit]]):
                sel = hit & (mesh_of[np.where(hit, i, 0)] == mesh)
                assert prim[sel].max() < slot_tables[mesh].size
                m[sel] = base[i[sel]] + slot_tables[mesh][prim[sel]]
            inst[s] = np.where(hit, i, NONE).astype(np.uint32)
            mat[s] = m
    finally:
        o.close()
    inst.flags.writeable = False
    mat.flags.writeable = False
    return inst, mat


# ---- the host build of pt_matte.h -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.mt_host_clear.argtypes = [C.c_void_p]
    L.mt_host_fold.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mt_host_coverage.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.mt_host_pick.argtypes = [C.c_void_p]
    L.mt_host_pick.restype = C.c_uint32
    L.mt_host_layout.argtypes = [C.POINTER(C.c_uint32 * 18)]
    return L


def host_fold(ids, state=None):
    """matte_fold over `ids`, from empty slots or from `state` ((SLOTS,) SLOT_DTYPE): the slots after."""
    ids = np.ascontiguousarray(ids, np.uint32)
    slots = np.empty(SLOTS, SLOT_DTYPE)
    if state is None:
        lib().mt_host_clear(slots.ctypes.data)
    else:
        slots[:] = state
    lib().mt_host_fold(ids.ctypes.data, ids.size, slots.ctypes.data)
    return slots


def host_coverage(slots, ids, n):
    slots = np.ascontiguousarray(slots, SLOT_DTYPE).reshape(-1, SLOTS)
    ids = np.ascontiguousarray(np.asarray(list(ids), np.uint32))
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.uint32), slots.shape[:1]))
    out = np.empty(slots.shape[0], np.float32)
    lib().mt_host_coverage(slots.ctypes.data, slots.shape[0], ids.ctypes.data if ids.size else None, ids.size, n.ctypes.data, out.ctypes.data)
    return out


def host_pick(slots):
    slots = np.ascontiguousarray(slots, SLOT_DTYPE)
    return int(lib().mt_host_pick(slots.ctypes.data))


def host_layout():
    o = (C.c_uint32 * 18)()
    lib().mt_host_layout(C.byref(o))
    return list(o)
