"""The transparent film without a GPU: the host build of pt_film.h (tests/emu/film_emu.cpp) against an independent float32
numpy restatement of the fold and of both compose modes, bit for bit; the properties the arithmetic promises; the ABI through libptamd.so;
and a stand-alone sanitizer build of the host code."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import film_lib as fl
from platinum_amd import abi

f32 = np.float32
INVALID = -1
NAN, INF = float("nan"), float("inf")
DENORMAL = float(np.finfo(np.float32).smallest_subnormal)


def _samples(seed, ns, npix):
    rng = np.random.default_rng(seed)
    L = np.concatenate([rng.gamma(0.7, 2.0, (ns, npix, 3)), np.ones((ns, npix, 1))], -1).astype(f32)
    hit = rng.random((ns, npix)) < 0.6
    hit[:, 0] = True           # pixel 0: every sample hits
    hit[:, 1] = False          # pixel 1: none does
    return L, hit


# ---- the fold ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [fl.KEEP, fl.ZERO])
@pytest.mark.parametrize("ns,n0", [(1, 0), (16, 0), (9, 0), (7, 9), (3, 1000), (8, 16777216)])
def test_host_fold_equals_the_numpy_restatement_bit_for_bit(ns, n0, policy):
    L, hit = _samples(ns * 31 + n0 % 97, ns, 40)
    start = None if n0 == 0 else np.random.default_rng(5).random((40, 4)).astype(f32)
    a = fl.host_fold(L, hit, policy, n0, start)
    b = fl.np_fold(L, hit, policy, n0, start)
    assert fl.same_bits(a, b), fl.first_difference(a, b)
    if n0 == 0:
        assert (a[0, 3] == 1.0) and not a[1].any()
        # all hit: the accumulator's own recurrence on rgb
        acc = np.zeros(3, f32)
        for s in range(ns):
            acc = L[s, 0, :3] if s == 0 else ((L[s, 0, :3] + acc * f32(s)) / f32(s + 1)).astype(f32)
        assert fl.same_bits(a[0, :3], acc)
        assert ((a[..., 3] >= 0) & (a[..., 3] <= 1)).all()


@pytest.mark.parametrize("policy", [fl.KEEP, fl.ZERO])
def test_the_film_does_not_depend_on_the_batching(policy):
    L, hit = _samples(3, 16, 64)
    L = L.copy()
    L[2, 5, 1] = NAN; hit[2, 5] = True
    L[4, 6, 0] = INF; hit[4, 6] = False
    whole = fl.host_fold(L, hit, policy)
    for split in ((7, 7, 2), (1,) * 16, (8, 8), (5, 11)):
        film, n0 = None, 0
        for nb in split:
            film = fl.host_fold(L[n0:n0 + nb], hit[n0:n0 + nb], policy, n0, film)
            n0 += nb
        assert n0 == 16 and fl.same_bits(film, whole), split
    assert fl.same_bits(whole, fl.np_fold(L, hit, policy))


@pytest.mark.parametrize("policy", [fl.KEEP, fl.ZERO])
@pytest.mark.parametrize("value", [NAN, INF, -INF, 3.2e38])
def test_a_non_finite_sample_on_a_hit_and_on_a_miss(value, policy):
    ns = 6
    L = np.full((ns, 2, 4), 0.5, f32)
    hit = np.ones((ns, 2), bool)
    L[3, 0, 1] = value                      # pixel 0: on a hit
    L[3, 1, 1] = value; hit[3, 1] = False   # pixel 1: on a miss
    a = fl.host_fold(L, hit, policy)
    assert fl.same_bits(a, fl.np_fold(L, hit, policy))
    # the miss contributes {0, 0, 0, 0} whatever its radiance: five samples of 0.5 and one of 0, coverage 5/6
    clean = L.copy(); clean[3, 1, :3] = 0
    assert fl.same_bits(a[1], fl.np_fold(clean, hit, policy)[1]) and np.isfinite(a[1]).all()
    assert a[1, 3] == fl.np_fold(clean, hit)[1, 3] and 0.83 < a[1, 3] < 0.84
    if policy == fl.ZERO:                   # the hit's radiance is zeroed as a whole (3.2e38 is past the product's 3.0e38 test too), its coverage stays
        zeroed = L.copy(); zeroed[3, 0, :3] = 0
        assert fl.same_bits(a[0], fl.np_fold(zeroed, hit, fl.KEEP)[0]) and a[0, 3] == 1.0
    else:
        assert not np.isfinite(a[0, 1]) or value == 3.2e38
        assert a[0, 0] == 0.5 and a[0, 3] == 1.0


# ---- the compose ---------------------------------------------------------------------------------------------------------------------------
ALPHAS = [0.0, 1.0, 1.0 / 3.0, DENORMAL, 0.5, NAN]
BACKDROPS = [(0.0, 0.0, 0.0), (1.0e30, 65504.0, 3.0e38), (0.18, 0.5, 1.0)]


def _card():
    """(base, film) (2, len(ALPHAS) * 3, 4): every alpha under three foreground colours, premultiplied."""
    a = np.repeat(np.array(ALPHAS, f32), 3)
    F = np.tile(np.array([[0.25, 1.5, 900.0], [0.0, 0.0, 0.0], [1.0e-30, 1.0, 3.0e38]], f32), (len(ALPHAS), 1))
    with np.errstate(all="ignore"):
        film = np.concatenate([(F * a[:, None]).astype(f32), a[:, None]], -1)
    film = np.stack([film, film[::-1]])
    base = film.copy()
    base[..., 3] = 1.0
    return base, film


@pytest.mark.parametrize("rgb", BACKDROPS)
@pytest.mark.parametrize("mode", [fl.COLOR, fl.TRANSPARENT])
def test_host_compose_equals_the_numpy_restatement_bit_for_bit(mode, rgb):
    base, film = _card()
    o = fl.options(enabled=1, backdrop=mode, backdrop_rgb=rgb)
    H, W = film.shape[:2]
    for rect in (None, (1, 0, W - 2, 1), (0, 1, 1, 2)):
        a = fl.host_compose(base, film, o, rect)
        b = fl.np_compose(base, film[..., 3], mode, rgb, rect)
        assert fl.same_bits(a, b), (rect, fl.first_difference(a, b))
        if rect is not None:
            inside = np.zeros((H, W), bool)
            inside[rect[1]:rect[3], rect[0]:rect[2]] = True
            assert not a[~inside].any()
    a = fl.host_compose(base, film, o)
    al = film[..., 3]
    if mode == fl.COLOR:
        assert (a[..., 3] == 1.0).all()
        assert fl.same_bits(a[al == 1.0][:, :3], base[al == 1.0][:, :3])                          # alpha 1: the foreground itself, + backdrop * 0
        if rgb != BACKDROPS[1]:
            assert fl.same_bits(a[al == 0.0][:, :3], np.broadcast_to(np.array(rgb, f32), a[al == 0.0][:, :3].shape))   # alpha 0: the backdrop
        if rgb == BACKDROPS[0]:
            ok = ~np.isnan(al)
            assert fl.same_bits(a[ok][:, :3], base[ok][:, :3] + f32(0))                            # backdrop 0: the premultiplied foreground
    else:
        assert fl.same_bits(a[..., 3], al)
        assert not a[~(al > 0)][:, :3].any()                                                       # alpha 0 and NaN: 0, never 0 / 0
        assert fl.same_bits(a[al == 1.0][:, :3], base[al == 1.0][:, :3])


def test_the_alpha_byte():
    alphas = np.array([0.0, -0.0, DENORMAL, 1.0 / 510.0 - 1e-6, 1.0 / 510.0 + 1e-6, 1.0 / 3.0, 0.5, 254.5 / 255.0 + 1e-6, 1.0, 1.5, INF, NAN, -1.0], f32)
    want = [0, 0, 0, 0, 1, 85, 128, 255, 255, 255, 255, 0, 0]
    assert fl.np_quantise(alphas).tolist() == want
    composed = np.zeros((1, alphas.size, 4), f32)
    composed[0, :, 3] = alphas
    target = np.random.default_rng(1).integers(0, 256, (1, alphas.size, 4), dtype=np.uint8)
    out = fl.host_alpha(target, composed)
    assert out[0, :, 3].tolist() == want and np.array_equal(out[..., :3], target[..., :3])
    every = (np.arange(256, dtype=f32) / f32(255)).astype(f32)                                    # the quantiser round-trips every byte
    assert fl.np_quantise(every).tolist() == list(range(256))


# ---- validation and surface ----------------------------------------------------------------------------------------------------------------
def test_film_options_abi():
    O = abi.FilmOptions
    assert fl.layout() == [C.sizeof(O)] + [getattr(O, n).offset for n, _ in O._fields_] == [20, 0, 4, 8]
    assert (abi.BACKDROP_SCENE, abi.BACKDROP_COLOR, abi.BACKDROP_TRANSPARENT) == (0, 1, 2)
    lib = abi.load_library()
    o = O(7, 7, (C.c_float * 3)(7, 7, 7))
    lib.pt_default_film_options(C.byref(o))
    assert (o.enabled, o.backdrop, list(o.backdrop_rgb)) == (0, abi.BACKDROP_SCENE, [0.0, 0.0, 0.0])
    assert bytes(o) == bytes(fl.options())
    lib.pt_default_film_options(None)


GOOD = [{}, dict(enabled=1), dict(backdrop=abi.BACKDROP_COLOR), dict(backdrop=abi.BACKDROP_TRANSPARENT), dict(backdrop_rgb=(0.0, 1.0e30, 3.4e38)),
        dict(enabled=1, backdrop=abi.BACKDROP_COLOR, backdrop_rgb=(0.2, 0.3, 0.4))]
BAD = [(dict(backdrop=3), b"backdrop"), (dict(backdrop=0xFFFFFFFF), b"backdrop")]
for _k in range(3):
    for _v in (-0.01, NAN, INF, -INF):
        _c = [0.5, 0.5, 0.5]
        _c[_k] = _v
        BAD.append((dict(backdrop_rgb=tuple(_c)), b"backdrop_rgb"))


def test_validation_before_the_renderer():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not."""
    lib = abi.load_library()
    for f in GOOD:
        o = fl.options(**f)
        assert fl.lib().film_host_options_valid(C.byref(o)) == 1
        assert lib.pt_set_film_options(None, C.byref(o)) == INVALID and b"null renderer" in lib.pt_last_error(), f
    for f, word in BAD:
        for en in (0, 1):
            o = fl.options(**f)
            o.enabled = en
            assert fl.lib().film_host_options_valid(C.byref(o)) == 0, f
            assert lib.pt_set_film_options(None, C.byref(o)) == INVALID and word in lib.pt_last_error(), f
    assert lib.pt_set_film_options(None, None) == INVALID
    out = np.zeros(4, np.float32)
    assert lib.pt_read_film(None, out.ctypes.data) == INVALID
    from platinum_amd.renderer import Renderer
    for member in ("filmOptions", "setFilmOptions", "readbackFilm"):
        assert callable(getattr(Renderer, member)), member


def test_the_queue_budget_counts_the_flag_buffer():
    """4 B per path slot beside the ~200 B of queue state: 204, 236 with AOVs (host_scene.h queue_budget through the host build)."""
    L = fl.lib()
    L.film_host_queue_budget.argtypes = [C.c_uint64] * 3 + [C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64]
    L.film_host_queue_budget.restype = C.c_uint64
    Q = L.film_host_queue_budget
    assert Q(1000, 0, 0, 0, 0, 0, 0, 0, 77) == 1000                      # the film off: Fbuf is not counted, nothing changes
    assert Q(2040, 0, 0, 0, 0, 0, 0, 1, 0) == 2000 and Q(203, 0, 0, 0, 0, 0, 0, 1, 0) == 0
    assert Q(2000, 0, 0, 0, 0, 0, 0, 1, 40) == 2000                       # what the previous render's Fbuf holds is reused
    assert Q(2360, 0, 0, 1, 0, 0, 0, 1, 0) == 2000                        # 236 with AOVs
    assert Q(2440, 0, 0, 1, 0, 1, 0, 1, 0) == 2000                        # 244 with AOVs and mattes
    assert Q(0, 5, 5, 1, 5, 1, 5, 1, 5) == 0                              # free memory unknown


# ---- the host code under sanitizers, stand-alone -------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/emu/film_emu.cpp with its own main: the fold over batch splits with non-finite samples, the compose over the edge alphas.
    (Nothing loaded into Python runs under a sanitizer.)"""
    exe = tmp_path / "film_emu_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DFILM_EMU_MAIN", "-o", str(exe), fl.SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.returncode, p.stderr[-2000:])
    assert "policy 1: film of pixel 2" in p.stdout and "backdrop 2 (1e+30 2 0.5)" in p.stdout
