"""Sun and sky without a GPU: the host build of pt_sky.h (tests/emu/sky_emu.cpp) against an independent float64 numpy
witness, the properties the model promises (where the sun stands, the disc's energy, exact scaling with the sun's intensity, vacuum,
disc off, mirror symmetry, the colours of day and of a low sun, finite and non-negative output), the refusals and the ABI through
libptamd.so."""
import ctypes as C
import math

import numpy as np
import pytest

import sky_lib as sl
from platinum_amd import abi

f32 = np.float32


_HOST = {}


def host(name, w, h, **over):
    """The host build's (image, stats, flags) of a case, computed once per process and left alone."""
    key = (name, w, h, tuple(sorted(over.items())))
    if key not in _HOST:
        o = sl.case_options(name, w, h)
        for k, v in over.items():
            setattr(o, k, v)
        img, st, flags = sl.host_sky(o, w, h)
        img.setflags(write=False)
        _HOST[key] = (img, st, flags)
    return _HOST[key]


# ---- the float32 bound ---------------------------------------------------------------------------------------------------------------------
def test_the_recorded_bound_is_four_times_the_float32_restatements_own_error():
    measured, left_out = sl.measure_float32_error()
    print("numpy float32 against float64: %.4g (recorded %.4g, bound %.4g); at most %.4f of a map left out"
          % (measured, sl.BOUNDS["measured"], sl.BOUNDS["bound"], left_out))
    assert sl.BOUNDS["bound"] == 4 * sl.BOUNDS["measured"]
    assert 0.99 * sl.BOUNDS["measured"] <= measured <= sl.BOUNDS["measured"]
    assert left_out <= sl.LEFT_OUT_CAP   # the sets are such that the restatement alone stays within the cap


# ---- host build against the float64 witness ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sl.OPTION_SETS))
def test_host_build_agrees_with_the_float64_witness(name):
    for w, h in sl.HOST_SIZES:
        wit = sl.witness(name, w, h)
        img, st, flags = host(name, w, h)
        assert np.isfinite(img).all() and (img >= 0).all() and (img[..., 3] == 1).all(), (w, h)
        ground, blocked = sl.unpack_flags(flags)
        mask = sl.compared(ground, blocked, wit)
        err = sl.rel_err(img, wit, mask)
        print("%s %d x %d: %.4g (bound %.4g), %.4f left out" % (name, w, h, err, sl.BOUNDS["bound"], 1 - mask.mean()))
        assert 1 - mask.mean() <= sl.LEFT_OUT_CAP, (w, h)
        assert err <= sl.BOUNDS["bound"], (w, h, err)
        # the stats: s, alpha_eff, Omega_d and the covered texels
        assert np.allclose(np.array(st.sun_direction[:]), wit["s"], rtol=0, atol=4e-7), (w, h)
        assert abs(st.sun_radius_used - wit["alpha_eff"]) <= 2e-7 * wit["alpha_eff"]
        cov = sl.host_coverage(sl.case_options(name, w, h), w, h)
        assert np.array_equal(cov, np.round(wit["coverage"] * 16).astype(np.uint32)), (w, h)
        assert abs(st.sun_solid_angle - wit["omega_d"]) <= 1e-12 * wit["omega_d"] and st.sun_texels == int((cov > 0).sum()), (w, h)


# ---- properties ----------------------------------------------------------------------------------------------------------------------------
def _sun_texel(o, w, h):
    col = (float(o.sun_azimuth) / (2 * math.pi) * w) % w
    row = (math.pi / 2 - float(o.sun_elevation)) / math.pi * h
    return int(col) % w, min(int(row), h - 1)


@pytest.mark.parametrize("name", ["default", "low-sun", "azimuth-negative", "azimuth-wrapped", "altitude-10"])
def test_the_brightest_texel_is_the_suns(name):
    for w, h in [(64, 32), (37, 19), (256, 128)]:
        img = host(name, w, h)[0]
        y, x = np.unravel_index(np.argmax(img[..., :3].sum(axis=-1)), (h, w))
        sx, sy = _sun_texel(sl.case_options(name, w, h), w, h)
        dx = min((x - sx) % w, (sx - x) % w)
        assert dx <= 1 and abs(int(y) - sy) <= 1, (w, h, (x, y), (sx, sy))


@pytest.mark.parametrize("w,h", [(64, 32), (256, 128), (37, 19)])
@pytest.mark.parametrize("name", ["default", "low-sun"])
def test_the_discs_irradiance_is_the_intensity_times_the_mean_transmittance(name, w, h):
    """sum of L_sun omega = I x the coverage-weighted mean of the witness's T(tau_view) (a covered texel of the ground counts as opaque),
    whatever the map's size: the division is by the discrete solid angle."""
    wit = sl.witness(name, w, h)
    on, off = host(name, w, h)[0], host(name, w, h, sun_disc=0)[0]
    sun = on[..., :3].astype(np.float64) - off[..., :3].astype(np.float64)
    got = (sun * wit["omega"][..., None]).sum(axis=(0, 1))
    weight = wit["coverage"] * wit["omega"]
    want = (np.where(wit["ground"][..., None], 0.0, wit["t_view"]) * weight[..., None]).sum(axis=(0, 1)) / weight.sum()
    print(name, w, h, got, want)
    assert np.all(np.abs(got - want) <= sl.BOUNDS["bound"] * want)
    if name == "low-sun":   # the light of a low sun has lost its blue
        assert got[0] > got[1] > got[2]


@pytest.mark.parametrize("name", ["default", "twilight", "altitude-10"])
def test_output_is_linear_in_the_suns_intensity_bit_for_bit_for_powers_of_two(name):
    base = host(name, 37, 19)[0]
    for scale in (4.0, 0.25, 1024.0):
        img = host(name, 37, 19, sun_intensity=scale)[0]
        want = base * f32(scale)
        want[..., 3] = 1
        assert np.array_equal(sl.bits(img), sl.bits(want)), scale
    assert np.all(host(name, 37, 19, sun_intensity=0.0)[0][..., :3] == 0)


def test_a_vacuum_has_a_black_sky_and_a_disc_of_intensity_over_solid_angle():
    for w, h in sl.HOST_SIZES:
        img, st, flags = host("vacuum", w, h, sun_intensity=2.0)
        ground = sl.unpack_flags(flags)[0]
        cov = sl.host_coverage(sl.case_options("vacuum", w, h), w, h)
        sky = ~ground
        assert (cov[sky] > 0).any() and np.all(img[sky & (cov == 0)][:, :3] == 0)
        want = (cov.astype(f32) * f32(0.0625) * f32(2.0)) / f32(st.sun_solid_angle)    # exactly: T = 1
        assert np.array_equal(sl.bits(img[sky][:, :3]), sl.bits(np.repeat(want[sky][:, None], 3, axis=1)))
        full = sky & (cov == 16)
        if full.any():
            assert np.allclose(img[full][:, :3], 2.0 / st.sun_solid_angle, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["default", "low-sun", "twilight", "zenith"])
def test_disc_off_equals_disc_on_where_nothing_is_covered(name):
    for w, h in sl.HOST_SIZES:
        on, off = host(name, w, h)[0], host(name, w, h, sun_disc=0)[0]
        cov = sl.host_coverage(sl.case_options(name, w, h), w, h)
        assert np.array_equal(sl.bits(on[cov == 0]), sl.bits(off[cov == 0])), (w, h)
        ground = sl.unpack_flags(host(name, w, h)[2])[0]
        assert np.all(on[(cov > 0) & ~ground][:, :3] >= off[(cov > 0) & ~ground][:, :3])
        assert host(name, w, h)[1].sun_solid_angle == host(name, w, h, sun_disc=0)[1].sun_solid_angle


@pytest.mark.parametrize("k", [0, 16, 23])
def test_the_sky_is_mirror_symmetric_about_a_sun_on_a_texel_boundary(k):
    w, h = 64, 32
    img = host("default", w, h, sun_azimuth=2 * math.pi * k / w)[0][..., :3].astype(np.float64)
    mirror = img[:, (2 * k - 1 - np.arange(w)) % w]
    floor = sl.FLOOR * img.max()
    err = np.abs(img - mirror) / np.maximum(np.abs(mirror), floor)
    print(k, err.max())
    assert err.max() <= sl.BOUNDS["bound"]


def test_the_sky_is_blue_by_day():
    for w, h in [(64, 32), (37, 19)]:
        img = host("disc-off", w, h)[0]
        r, g, b = img[: h // 2, :, :3].astype(np.float64).mean(axis=(0, 1))
        assert b > g > r > 0, (r, g, b)


# ---- refusals and the ABI ------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = [{}, dict(sun_elevation=-math.pi / 2), dict(sun_elevation=math.pi / 2), dict(sun_azimuth=-1e30), dict(sun_azimuth=3e38),
        dict(sun_angular_radius=0.2), dict(sun_angular_radius=1e-6), dict(sun_intensity=0.0), dict(sun_intensity=3e38), dict(sun_disc=0),
        dict(altitude_km=0.001), dict(altitude_km=60.0), dict(air_density=0.0), dict(air_density=10.0), dict(dust_density=10.0),
        dict(ozone_density=10.0), dict(ground_albedo=0.0), dict(ground_albedo=1.0)]
BAD = [(dict(sun_elevation=1.6), b"sun_elevation"), (dict(sun_elevation=-1.6), b"sun_elevation"), (dict(sun_elevation=NAN), b"sun_elevation"),
       (dict(sun_azimuth=NAN), b"sun_azimuth"), (dict(sun_azimuth=INF), b"sun_azimuth"), (dict(sun_azimuth=-INF), b"sun_azimuth"),
       (dict(sun_angular_radius=0.0), b"sun_angular_radius"), (dict(sun_angular_radius=0.21), b"sun_angular_radius"),
       (dict(sun_angular_radius=NAN), b"sun_angular_radius"), (dict(sun_angular_radius=-0.1), b"sun_angular_radius"),
       (dict(sun_intensity=-1.0), b"sun_intensity"), (dict(sun_intensity=INF), b"sun_intensity"), (dict(sun_intensity=NAN), b"sun_intensity"),
       (dict(sun_disc=2), b"sun_disc"),
       (dict(altitude_km=0.0), b"altitude_km"), (dict(altitude_km=60.5), b"altitude_km"), (dict(altitude_km=NAN), b"altitude_km"),
       (dict(air_density=-0.1), b"air_density"), (dict(air_density=10.5), b"air_density"), (dict(air_density=NAN), b"air_density"),
       (dict(dust_density=-0.1), b"dust_density"), (dict(dust_density=10.5), b"dust_density"), (dict(dust_density=NAN), b"dust_density"),
       (dict(ozone_density=-0.1), b"ozone_density"), (dict(ozone_density=10.5), b"ozone_density"), (dict(ozone_density=NAN), b"ozone_density"),
       (dict(ground_albedo=-0.1), b"ground_albedo"), (dict(ground_albedo=1.1), b"ground_albedo"), (dict(ground_albedo=NAN), b"ground_albedo")]
BAD_SIZES = [(0, 4), (4, 0), (1 << 13, (1 << 13) + 1), (1 << 31, 1 << 31), (0xFFFFFFFF, 0xFFFFFFFF)]


def test_every_invalid_option_and_size_is_refused_before_the_renderer():
    lib = abi.load_library()
    out = np.zeros((4, 8, 4), np.float32)
    gen = lambda o, w, h: lib.pt_generate_sky(None, C.byref(o), w, h, out.ctypes.data, None)
    for f in GOOD:
        o = sl.options(**f)
        assert sl.lib().sk_host_valid(C.byref(o), 8, 4) == 1, f
        assert gen(o, 8, 4) == -1 and b"null renderer" in lib.pt_last_error(), f      # a valid struct reaches the renderer's test
    for f, word in BAD:
        o = sl.options(**f)
        assert sl.lib().sk_host_valid(C.byref(o), 8, 4) == 0, f
        assert sl.lib().sk_host_generate(C.byref(o), 8, 4, out.ctypes.data, None, None) == -1, f
        assert gen(o, 8, 4) == -1 and word in lib.pt_last_error(), f                   # PT_ERR_INVALID_ARGUMENT, and why
    o = sl.options()
    for w, h in BAD_SIZES:
        assert sl.lib().sk_host_valid(C.byref(o), w, h) == 0, (w, h)
        assert gen(o, w, h) == -1 and b"texels" in lib.pt_last_error(), (w, h)
    assert sl.lib().sk_host_valid(C.byref(o), 1 << 13, 1 << 13) == 1 and gen(o, 1 << 13, 1 << 13) == -1 and b"null renderer" in lib.pt_last_error()
    assert lib.pt_generate_sky(None, None, 8, 4, out.ctypes.data, None) == -1 and b"null argument" in lib.pt_last_error()
    assert lib.pt_generate_sky(None, C.byref(o), 8, 4, None, None) == -1 and b"null argument" in lib.pt_last_error()


def test_any_finite_azimuth_and_the_extreme_options_give_a_finite_image():
    for f in GOOD:
        o = sl.options(**f)
        img, st, _ = sl.host_sky(o, 16, 8)
        assert np.isfinite(img).all() and (img >= 0).all() and (img[..., 3] == 1).all(), f
        assert abs(np.linalg.norm(st.sun_direction[:]) - 1) < 1e-6, f
    # a map so coarse in one direction that no sub-texel direction may fall inside the disc still holds a finite sky
    img, st, _ = sl.host_sky(sl.options(sun_azimuth=0.8), 1, 64)
    assert np.isfinite(img).all() and (st.sun_texels > 0) == (st.sun_solid_angle > 0)


def test_the_defaults_and_the_layout_are_the_headers():
    lib = abi.load_library()
    o = abi.SkyOptions(*([7] * 10))
    lib.pt_default_sky_options(C.byref(o))
    d = sl.options()
    assert bytes(o) == bytes(d)
    assert (o.sun_elevation, o.sun_azimuth, o.sun_disc) == (0.5, 0.0, 1) and o.sun_angular_radius == f32(0.004712) and o.altitude_km == f32(0.001)
    lib.pt_default_sky_options(None)
    got = sl.layout()
    want = [C.sizeof(abi.SkyOptions)] + [getattr(abi.SkyOptions, n).offset for n, _ in abi.SkyOptions._fields_]
    want += [C.sizeof(abi.SkyStats)] + [getattr(abi.SkyStats, n).offset for n, _ in abi.SkyStats._fields_]
    assert got == want and got[0] == 40 and got[11] == 32
