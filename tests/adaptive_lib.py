"""Host side of the adaptive-sampling tests: the ctypes wrapper of the ad_* functions of the host harness (tests/host_build.py; the host build of
platinum_amd/csrc/pt_adaptive.h and of the denoiser's per-pixel-N prep, tests/emu/adaptive_emu.cpp) and a float64 numpy restatement of
the criterion as DESIGN.md §3b states it; reference_render, a whole adaptive render on the host (denoise_lib.HostScene + the host
criterion), and the configurations tests/test_adaptive_reference.py and tests/test_gpu_adaptive_matrix.py share.  TEST HARNESS, never
imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import host_build  # noqa: E402

LUM_FLOOR = 1e-3


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load()
    L.ad_host_error.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.ad_host_tiles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    L.ad_host_filter_counts.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 2 + [C.c_void_p, C.c_uint32] + [C.c_float] * 3 + [C.c_void_p]
    L.ad_host_options_layout.argtypes = [C.POINTER(C.c_uint32 * 5)]
    return L


def host_error(m1, m2, n):
    m1, m2 = np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)
    err = np.zeros(m1.shape, np.float32)
    lib().ad_host_error(m1.ctypes.data, m2.ctypes.data, m1.size, n, err.ctypes.data)
    return err


def host_tiles(moments, n, threshold):
    """(tilesY, tilesX) bool: the tiles of a (H, W, 4) PT_AOV_MOMENTS image that converge after n samples."""
    moments = np.ascontiguousarray(moments, np.float32)
    H, W = moments.shape[:2]
    out = np.zeros(((H + 7) // 8, (W + 7) // 8), np.uint8)
    lib().ad_host_tiles(moments.ctypes.data, W, H, n, threshold, out.ctypes.data)
    return out.astype(bool)


def host_filter_counts(acc, albedo, normal, moments, counts, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    """The denoiser of an adaptive render (per-pixel N = counts, (H, W) uint32) built for the host."""
    imgs = [np.ascontiguousarray(x, np.float32) for x in (acc, albedo, normal, moments)]
    counts = np.ascontiguousarray(counts, np.uint32)
    H, W = imgs[0].shape[:2]
    out = np.zeros((H, W, 4), np.float32)
    lib().ad_host_filter_counts(*[x.ctypes.data for x in imgs], W, H, counts.ctypes.data, iterations, sigma_l, sigma_n, sigma_z, out.ctypes.data)
    return out


def options_layout():
    o = (C.c_uint32 * 5)()
    lib().ad_host_options_layout(C.byref(o))
    return list(o)


def same_bits_or_both_nan(a, b):
    """Per component: the same bits, or NaN on both sides (the payload of a NaN is not compared; an inf against a NaN differs)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- float64 restatement ----------------------------------------------------------------------------------------------
def np_error(m1, m2, n):
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    with np.errstate(all="ignore"):
        var = np.maximum(m2 - m1 * m1, 0.0) * n / (n - 1)
        return np.sqrt(var / n) / np.maximum(m1, LUM_FLOOR)


def np_converged(m1, m2, n, threshold):
    if n < 2:
        return np.zeros(np.shape(m1), bool)
    with np.errstate(invalid="ignore"):
        return np_error(m1, m2, n) <= threshold


def tile_view(img, H, W):
    """(tilesY, tilesX) list of the tiles' slices of an (H, W, ...) image."""
    return [[(slice(ty * 8, min(H, ty * 8 + 8)), slice(tx * 8, min(W, tx * 8 + 8))) for tx in range((W + 7) // 8)] for ty in range((H + 7) // 8)]


# ---- a whole adaptive render on the host, no GPU in the loop ------------------------------------------------------------
def checkpoints(spp, min_spp, interval):
    """The sample counts at which a render of `spp` samples takes a verdict: min_spp, min_spp + interval, ... below spp."""
    return list(range(min_spp, spp, interval))


def reference_render(scene, params, threshold, min_spp, interval, stop_at=None, trace=None, info=None):
    """The adaptive render of `scene` under `params` (spp, first_sample, integrator, ... as the device gets them) on the host build of the
    product's stage functions (denoise_lib.HostScene): samples are folded cumulatively, the host build of the criterion (host_tiles)
    judges the moments at every checkpoint below spp, and a tile's accumulator, AOVs and count freeze at the first checkpoint where it
    converges.  Returns (counts (H, W) uint32, acc, albedo, normal, moments).  `stop_at` = n: the state after n samples (active tiles
    hold n).  `trace`, a list, receives (checkpoint, moments at it, tiles active before it) per checkpoint.  `info`, a dict, receives
    "nonfinite": (H, W) uint32, the NaN / inf samples among those each pixel's tile drew (params.nonfinite_policy decides what they did to
    the images; a sample a stopped tile never drew does not count)."""
    import denoise_lib as dl
    hs = dl.HostScene(scene, params)
    H, W = hs.H, hs.W
    spp, first = int(params.spp), int(params.first_sample)
    end = spp if stop_at is None else min(int(stop_at), spp)
    live = [np.zeros((H, W, 4), np.float32) for _ in range(4)]
    out = [np.zeros((H, W, 4), np.float32) for _ in range(4)]
    counts = np.zeros((H, W), np.uint32)
    live_nf, out_nf = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    active = np.ones(((H + 7) // 8, (W + 7) // 8), bool)
    tv = tile_view(counts, H, W)

    def freeze(tiles, n):
        for ty, tx in zip(*np.nonzero(tiles)):
            s = tv[ty][tx]
            counts[s] = n
            for o, l in zip(out + [out_nf], live + [live_nf]):
                o[s] = l[s]

    done = 0
    cps = checkpoints(spp, min_spp, interval)
    for c in sorted(set([c for c in cps if c <= end] + [end])):
        if c > done:
            hs.render(first + done, c - done, n0=done, into=live, nonfinite=live_nf)
            done = c
        if c in cps and active.any():
            if trace is not None:
                trace.append((c, live[3].copy(), active.copy()))
            conv = host_tiles(live[3], c, threshold) & active
            freeze(conv, c)
            active &= ~conv
    freeze(active, end)
    if info is not None:
        info["nonfinite"] = out_nf
    return (counts,) + tuple(out)


def tile_counts(counts):
    return counts[::8, ::8]


def check_populated(counts, spp, W, H):
    """The preconditions of a comparison with a reference: every class of tile takes part (else it could pass vacuously)."""
    tc = tile_counts(counts)
    assert np.array_equal(np.kron(tc, np.ones((8, 8), np.uint32))[:H, :W], counts)
    distinct = sorted(set(tc.ravel().tolist()))
    assert len(distinct) >= 5 and distinct[-1] == spp, distinct
    early = float((tc < spp).mean())
    assert 0.15 <= early <= 0.85, early
    assert W % 8 and H % 8
    edge = np.zeros(tc.shape, bool)
    edge[-1, :] = edge[:, -1] = True     # the partial tiles
    assert (tc[edge] < spp).any() and (tc[edge] == spp).any()
    # (stopped early in the last tile row) + (in the last tile column): the corner tile counts in both
    return distinct, early, int((tc[-1, :] < spp).sum() + (tc[:, -1] < spp).sum())


def histogram(counts):
    tc = tile_counts(counts)
    return ", ".join("%d: %d" % (n, int((tc == n).sum())) for n in sorted(set(tc.ravel().tolist()))) + " (of %d)" % tc.size


# ---- the configurations the reference tests and the GPU matrix share -------------------------------------------------------------------
# scene, (W, H), bounces, spp, min_spp, interval, threshold: every count class is populated and partial edge tiles stop early and late
CONFIGS = {
    "cornell131": ("cornell", (131, 93), 4, 128, 16, 16, 0.2),
    "cornell67": ("cornell", (67, 45), 4, 96, 5, 7, 0.3),
    "textured99": ("textured", (99, 53), 6, 64, 8, 8, 0.5),
}


# The same, on the seeded random scenes that yield NaN samples at 71x45 with 3 + seed % 7 bounces (kind = "random<seed>"), with the
# nonfinite_policy (platinum_amd.abi.NONFINITE_*: 0 propagate, 1 zero) as an eighth field.  Their tiles are not spread over the count
# classes as check_populated asks: tests/test_adaptive_reference.py states and asserts what each of them is there for.
NONFINITE_CONFIGS = {
    "nan996": ("random996", (71, 45), 5, 48, 4, 4, 1.0, 0),
    "nan996_early": ("random996", (71, 45), 5, 48, 4, 4, 2.0, 0),
    "nan24": ("random24", (71, 45), 6, 24, 2, 2, 0.3, 0),
    "nan648": ("random648", (71, 45), 7, 32, 2, 3, 0.6, 0),
    "zero996": ("random996", (71, 45), 5, 48, 4, 4, 1.0, 1),
    "zero648": ("random648", (71, 45), 7, 32, 2, 3, 0.8, 1),
}


def config(name):
    """(kind, (W, H), bounces, spp, min_spp, interval, threshold, nonfinite_policy) of CONFIGS[name] or NONFINITE_CONFIGS[name]."""
    return CONFIGS[name] + (0,) if name in CONFIGS else NONFINITE_CONFIGS[name]


@functools.lru_cache(maxsize=None)
def config_scene(kind):
    from platinum_amd import scenes
    if kind.startswith("random"):
        return scenes.random_scene(int(kind[6:]))
    return scenes.cornell_scene("bench") if kind == "cornell" else scenes.textured_scene()


def config_params(name, first_sample=0, integrator=None):
    from platinum_amd import abi
    from platinum_amd.renderer import make_params
    _kind, (W, H), B, spp, _m, _i, _t, policy = config(name)
    return make_params(W, H, spp, B, first_sample=first_sample, integrator=abi.INTEGRATOR_MIS if integrator is None else integrator,
                       nonfinite_policy=policy)


@functools.lru_cache(maxsize=None)
def reference(name, min_spp=None, interval=None, first_sample=0, integrator=None, stop_at=None):
    """reference_render of CONFIGS[name] / NONFINITE_CONFIGS[name], once per process: a dict of counts / acc / albedo / normal / moments /
    trace / nonfinite (read only)."""
    kind, _size, _B, _spp, m, i, thr, _policy = config(name)
    m, i = (m, i) if min_spp is None else (min_spp, interval)
    trace, info = [], {}
    out = reference_render(config_scene(kind), config_params(name, first_sample, integrator), thr, m, i, stop_at=stop_at, trace=trace, info=info)
    for a in out + (info["nonfinite"],):
        a.flags.writeable = False
    return dict(zip(("counts", "acc", "albedo", "normal", "moments"), out), trace=trace, nonfinite=info["nonfinite"])


# ---- what the non-finite configurations are there for ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_nonfinite_samples(name):
    """The (sample, x, y) of every NaN / inf sample the oracle finds among the spp samples of NONFINITE_CONFIGS[name], one sample at a
    time under PT_NONFINITE_PROPAGATE (first_sample 0, MIS)."""
    import oracle_lib
    from platinum_amd.renderer import make_params
    kind, (W, H), B, spp, _m, _i, _t, _policy = config(name)
    o = oracle_lib.OracleScene(config_scene(kind), make_params(W, H, spp, B))
    try:
        out = []
        for s in range(spp):
            bad = ~np.isfinite(o.render(s, 1)[..., :3]).all(axis=-1)
            out += [(s, int(x), int(y)) for y, x in np.argwhere(bad)]
        assert o.stats().nonfinite == len(out)
    finally:
        o.close()
    return tuple(out)


def check_nonfinite_reference(name, ref):
    """Conditions (a), (b), (e) on the reference of NONFINITE_CONFIGS[name]; returns what (c) and (d) are decided from over the whole
    table: (count classes, tiles that stopped before their first non-finite sample and are finite everywhere, non-finite pixels that lie
    in a partial edge tile and were drawn)."""
    _kind, (W, H), _B, spp, _m, _i, _t, policy = config(name)
    counts, acc, mom = ref["counts"], ref["acc"], ref["moments"]
    tc = tile_counts(counts)
    assert np.array_equal(np.kron(tc, np.ones((8, 8), np.uint32))[:H, :W], counts) and W % 8 and H % 8
    samples = oracle_nonfinite_samples(name)
    drawn = [(s, x, y) for s, x, y in samples if s < counts[y, x]]
    # (a) the oracle sees a non-finite sample among the samples this render draws; and the reference counted exactly those
    assert len(drawn) >= 1, samples
    want = np.zeros((H, W), np.uint32)
    for _s, x, y in drawn:
        want[y, x] += 1
    assert np.array_equal(ref["nonfinite"], want)
    tv = tile_view(counts, H, W)
    if policy == 0:
        # (b) a tile that drew a non-finite sample can pass no later checkpoint; its pixel is NaN in acc and in the luminance moments
        for _s, x, y in drawn:
            assert counts[y, x] == spp, (x, y)
            assert np.isnan(acc[y, x, :3]).all() and acc[y, x, 3] == 1.0
            assert np.isfinite(mom[y, x, 0]) and np.isnan(mom[y, x, 1]) and np.isnan(mom[y, x, 2]) and mom[y, x, 3] == 0.0
        assert int(np.isnan(acc).any(axis=-1).sum()) == len({(x, y) for _s, x, y in drawn})
    else:
        # (e) zeroed samples leave everything finite, and there was one to zero
        assert np.isfinite(acc).all() and np.isfinite(mom).all() and int(ref["nonfinite"].sum()) >= 1
    assert np.isfinite(ref["albedo"]).all() and np.isfinite(ref["normal"]).all()
    spared, edge = [], []
    for s, x, y in samples:
        t = tv[y // 8][x // 8]
        first = min(s2 for s2, x2, y2 in samples if (y2 // 8, x2 // 8) == (y // 8, x // 8))
        if counts[y, x] <= first and np.isfinite(acc[t]).all() and np.isfinite(mom[t]).all():
            spared.append((y // 8, x // 8))
        if s < counts[y, x] and (y // 8 == (H - 1) // 8 or x // 8 == (W - 1) // 8):
            edge.append((x, y))
    return sorted(set(tc.ravel().tolist())), sorted(set(spared)), edge


def check_nonfinite_table(facts):
    """Conditions (c) and (d) over {name: check_nonfinite_reference(name, ...)} of every NONFINITE_CONFIGS entry."""
    assert set(facts) == set(NONFINITE_CONFIGS)
    assert any(spared for _c, spared, _e in facts.values())                              # (c)
    assert any(len(classes) >= 5 and edge for classes, _s, edge in facts.values())       # (d)
