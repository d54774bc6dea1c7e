"""Shared pieces of the post-process and GMoN resolve tests — TEST INFRASTRUCTURE.

  * RANGES: the range of every field of pt_post_options / pt_tonemap_options, the option sweep built from it (both ends of every field,
    64 seeded random combinations per tonemapper) and the three output spaces;
  * test cards (synthetic accumulators) and the regimes they must contain;
  * PRECISION / BOUND: what single precision costs the chain, measured with post_ref alone, and the bound derived from it;
  * the RGBA8 rule: bytes equal the quantised reference, or differ by exactly 1 next to a rounding boundary;
  * a float32 numpy restatement of the GMoN resolve, and a float64 evaluation of the quantities it is meant to compute;
  * the emissive-patch scene that puts a test card into the device's accumulator.
"""
import ctypes as C

import numpy as np

import post_ref
from platinum_amd import abi, scenes

f32 = np.float32

# ---- option ranges --------------------------------------------------------------------------------------------------------------------
# (low, high, where the range comes from).  "ui" = the drag widget of the reference's render viewport (pt_viewport.cpp:255-537), which is
# the only place the reference bounds these fields; "colour" = its colour picker, components in [0, 1]; "chosen" = the reference has no
# widget for the field (the gamut extension is only ever set by a preset, postprocessing.hpp:109-165): the range is this suite's choice,
# wide enough to hold both presets and to move every sextant of the hue rotation.  A vector field has the range per component.
POST_RANGES = {
    "exposure": (-5.0, 5.0, "ui"), "ca_amount": (-100.0, 100.0, "ui"), "ca_green_shift": (-100.0, 100.0, "ui"),
    "contrast": (-100.0, 100.0, "ui"), "saturation": (-100.0, 100.0, "ui"),
    "blacks": (-100.0, 100.0, "ui"), "shadows": (-100.0, 100.0, "ui"), "highlights": (-100.0, 100.0, "ui"), "whites": (-100.0, 100.0, "ui"),
    "vig_amount": (-5.0, 5.0, "ui"), "vig_midpoint": (-100.0, 100.0, "ui"), "vig_feather": (0.0, 100.0, "ui"),
    "vig_power": (0.0, 100.0, "ui"), "vig_roundness": (0.0, 100.0, "ui"),
}
GRADE_RANGES = {   # lift / gamma / gain: applied after every tonemapper
    "shadow_color": (0.0, 1.0, "colour"), "midtone_color": (0.0, 1.0, "colour"), "highlight_color": (0.0, 1.0, "colour"),
    "shadow_offset": (-100.0, 100.0, "ui"), "midtone_offset": (-100.0, 100.0, "ui"), "highlight_offset": (-100.0, 100.0, "ui"),
}
TONEMAPPER_RANGES = {
    abi.TONEMAP_NONE: {},
    abi.TONEMAP_AGX: {"agx_offset": (-10.0, 10.0, "ui"), "agx_slope": (-5.0, 5.0, "ui"), "agx_power": (0.0, 5.0, "ui"),
                      "agx_saturation": (0.0, 3.0, "ui")},
    abi.TONEMAP_KHRONOS_PBR: {"khr_compression_start": (0.2, 1.0, "ui"), "khr_desaturation": (0.0, 1.0, "ui")},
    abi.TONEMAP_FLIM: {
        "flim_pre_exposure": (-10.0, 10.0, "ui"), "flim_pre_formation_filter": (0.0, 1.0, "colour"),
        "flim_pre_formation_filter_strength": (0.0, 1.0, "ui"),
        "flim_extended_gamut_scale": (1.0, 1.5, "chosen"), "flim_extended_gamut_rotation": (-30.0, 30.0, "chosen"),
        "flim_extended_gamut_mul": (0.8, 1.25, "chosen"),
        "flim_sigmoid_log2_min": (-20.0, 50.0, "ui"), "flim_sigmoid_log2_max": (-20.0, 50.0, "ui"),
        "flim_sigmoid_toe": (0.0, 1.0, "ui"), "flim_sigmoid_shoulder": (0.0, 1.0, "ui"),
        "flim_negative_exposure": (-10.0, 10.0, "ui"), "flim_negative_density": (0.0, 100.0, "ui"),
        "flim_print_backlight": (0.0, 1.0, "colour"), "flim_print_exposure": (-10.0, 10.0, "ui"), "flim_print_density": (0.0, 100.0, "ui"),
        "flim_black_point": (0.0, 1.0, "ui"), "flim_auto_black_point": (0, 1, "checkbox"),
        "flim_post_formation_filter": (0.0, 1.0, "colour"), "flim_post_formation_filter_strength": (0.0, 1.0, "ui"),
        "flim_midtone_saturation": (0.0, 10.0, "ui"),
    },
}
TONEMAPPERS = (abi.TONEMAP_NONE, abi.TONEMAP_AGX, abi.TONEMAP_KHRONOS_PBR, abi.TONEMAP_FLIM)
TONEMAPPER_NAMES = {abi.TONEMAP_NONE: "none", abi.TONEMAP_AGX: "agx", abi.TONEMAP_KHRONOS_PBR: "khronos", abi.TONEMAP_FLIM: "flim"}
OUTPUT_SPACES = {"bt2020": scenes.BT2020, "display_p3": scenes.DISPLAY_P3, "bt709": scenes.BT709}   # BT.2020 is the working space: identity
RANDOM_PER_TONEMAPPER = 64


def defaults():
    lib = abi.load_library()
    po, to = abi.PostOptions(), abi.TonemapOptions()
    lib.pt_default_post_options(C.byref(po))
    lib.pt_default_tonemap_options(C.byref(to))
    return po, to


def _field_len(struct_type, name):
    t = dict(struct_type._fields_)[name]
    return getattr(t, "_length_", 0)


def _set(struct, name, value, index=None):
    if index is None:
        setattr(struct, name, value)
    else:
        getattr(struct, name)[index] = value


class Config:
    """One option set: a name and the assignments that lead to it from the defaults."""

    def __init__(self, name, tonemapper, post=(), tonemap=(), space="display_p3"):
        self.name, self.tonemapper, self.post, self.tonemap, self.space = name, tonemapper, tuple(post), tuple(tonemap), space

    def structs(self):
        po, to = defaults()
        to.tonemapper = self.tonemapper
        to.output_space = scenes.colorspace(OUTPUT_SPACES[self.space])
        for name, index, value in self.post:
            _set(po, name, value, index)
        for name, index, value in self.tonemap:
            _set(to, name, value, index)
        return po, to

    def __repr__(self):
        return self.name


def end_configs(tm):
    """The defaults, every output space, and every field that acts under tonemapper `tm` at both ends of its range, one at a time.
    flim_black_point only acts with the auto black point off, so its two ends are run that way."""
    tn = TONEMAPPER_NAMES[tm]
    out = [Config("%s/defaults" % tn, tm)]
    out += [Config("%s/space=%s" % (tn, s), tm, space=s) for s in OUTPUT_SPACES if s != "display_p3"]
    for name, (lo, hi, _src) in POST_RANGES.items():
        out += [Config("%s/%s=%g" % (tn, name, v), tm, post=[(name, None, v)]) for v in (lo, hi)]
    for ranges in (GRADE_RANGES, TONEMAPPER_RANGES[tm]):
        for name, (lo, hi, _src) in ranges.items():
            n = _field_len(abi.TonemapOptions, name)
            extra = [("flim_auto_black_point", None, 0)] if name == "flim_black_point" else []
            for index in (range(n) if n else [None]):
                for v in (lo, hi):
                    label = "%s/%s%s=%g" % (tn, name, "" if index is None else "[%d]" % index, v)
                    out.append(Config(label, tm, tonemap=extra + [(name, index, v)]))
    return out


def random_configs(tm, count=RANDOM_PER_TONEMAPPER):
    """`count` seeded draws of every field that acts under `tm` (uniform over its range; float32 values, as the structs hold them)."""
    rng = np.random.default_rng(20240 + int(tm))
    out = []
    for k in range(count):
        post = [(name, None, float(f32(rng.uniform(lo, hi)))) for name, (lo, hi, _s) in POST_RANGES.items()]
        tone = []
        for ranges in (GRADE_RANGES, TONEMAPPER_RANGES[tm]):
            for name, (lo, hi, src) in ranges.items():
                n = _field_len(abi.TonemapOptions, name)
                for index in (range(n) if n else [None]):
                    tone.append((name, index, int(rng.integers(0, 2)) if src == "checkbox" else float(f32(rng.uniform(lo, hi)))))
        space = list(OUTPUT_SPACES)[int(rng.integers(0, len(OUTPUT_SPACES)))]
        out.append(Config("%s/random%02d" % (TONEMAPPER_NAMES[tm], k), tm, post=post, tonemap=tone, space=space))
    return out


def sweep(tm):
    return end_configs(tm) + random_configs(tm)


# ---- test cards -----------------------------------------------------------------------------------------------------------------------
MID_GREY = 0.18
STOPS = 22.0                      # the log-uniform part spans MID_GREY * 2^(-11 .. +11)
CARD_SIZES = [(64, 48), (48, 64), (32, 32), (1, 1), (1, 37), (37, 1)]     # (W, H): landscape, portrait (aspect < 1), square, all taps clamp
KHRONOS_START = 0.8 - 0.04        # where the default Khronos curve starts to compress the peak


def special_pixels():
    """The pixels every card with room for them carries, each regime as a block of three: name -> [3, 3] colours."""
    out = {"black": [(0.0, 0.0, 0.0)] * 3}
    out["two_zero"] = [(0.31, 0.0, 0.0), (0.0, 0.47, 0.0), (0.0, 0.0, 0.9)]
    out["one_zero"] = [(0.31, 0.2, 0.0), (0.0, 0.47, 0.11), (0.6, 0.0, 0.9)]
    out["max_r"] = [(0.5, 0.2, 0.1), (0.09, 0.02, 0.05), (2.5, 1.0, 2.0)]
    out["max_g"] = [(0.2, 0.5, 0.1), (0.02, 0.09, 0.05), (1.0, 2.5, 2.0)]
    out["max_b"] = [(0.2, 0.1, 0.5), (0.02, 0.05, 0.09), (1.0, 2.0, 2.5)]
    out["max_rg"] = [(0.5, 0.5, 0.1), (0.05, 0.05, 0.01), (2.0, 2.0, 0.7)]
    out["max_rb"] = [(0.5, 0.1, 0.5), (0.05, 0.01, 0.05), (2.0, 0.7, 2.0)]
    out["max_gb"] = [(0.1, 0.5, 0.5), (0.01, 0.05, 0.05), (0.7, 2.0, 2.0)]
    out["grey"] = [(0.18, 0.18, 0.18), (0.02, 0.02, 0.02), (3.0, 3.0, 3.0)]
    out["luma_lt_0.04"] = [(0.01, 0.02, 0.03), (0.03, 0.03, 0.03), (0.001, 0.002, 0.05)]
    out["luma_0.04_0.18"] = [(0.05, 0.06, 0.07), (0.1, 0.1, 0.1), (0.3, 0.1, 0.1)]
    out["luma_0.18_0.75"] = [(0.2, 0.3, 0.4), (0.5, 0.5, 0.5), (0.9, 0.6, 0.2)]
    out["luma_gt_0.75"] = [(0.8, 0.9, 1.0), (1.5, 0.8, 0.4), (0.2, 1.1, 0.3)]
    out["khronos_below"] = [(0.5, 0.3, 0.2), (0.7, 0.7, 0.7), (0.3, 0.74, 0.1)]
    out["khronos_above"] = [(0.9, 0.3, 0.2), (2.0, 2.0, 2.0), (0.3, 0.85, 40.0)]
    lo, hi = MID_GREY * 2.0 ** (-STOPS / 2), MID_GREY * 2.0 ** (STOPS / 2)      # both ends of the span, so that every card reaches them
    out["darkest"] = [(lo, lo, lo), (lo, 0.5 * lo, 0.25 * lo), (0.5 * lo, lo, lo)]
    out["brightest"] = [(hi, hi, hi), (hi, 0.5 * hi, 0.25 * hi), (0.5 * hi, hi, hi)]
    return {k: np.array(v, dtype=f32) for k, v in out.items()}


def card(w, h, seed=0):
    """A synthetic accumulator [h, w, 4]: luminance log-uniform over STOPS stops around mid-grey times a random chroma in (0.05, 1], with
    the special pixels on a seeded selection of places as far as there is room (a 1x1 card is one mid-tone pixel)."""
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    level = MID_GREY * np.exp2(rng.uniform(-STOPS / 2, STOPS / 2, size=n))
    chroma = rng.uniform(0.05, 1.0, size=(n, 3))
    chroma /= chroma.max(axis=1, keepdims=True)
    rgb = (level[:, None] * chroma).astype(f32)
    if n == 1:
        rgb[0] = (0.31, 0.18, 0.07)
    else:
        special = np.concatenate(list(special_pixels().values()))
        # the long cards take one pixel of each regime, the others all three
        special = special if n >= len(special) else special[::3]
        where = rng.permutation(n)[:len(special)]
        rgb[where[:len(special)]] = special[:len(where)]
    acc = np.ones((h, w, 4), dtype=f32)
    acc[..., :3] = rgb.reshape(h, w, 3)
    return acc


def _luma(rgb):
    return rgb[..., 0] * 0.2126 + rgb[..., 1] * 0.7152 + rgb[..., 2] * 0.0722


def regimes(rgb, zero=0.0):
    """How many pixels of [..., 3] fall into each regime the cards must contain (all must be > 0 on a card with room for them).
    A channel counts as zero up to `zero` times the pixel's largest: the rendered card's zeros are 1e-17 of the lit channel, because
    the renderer's input transform of a BT.709 working space is inverse(M) * M in float, not the identity."""
    rgb = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    rgb = np.where(np.abs(rgb) <= zero * np.abs(rgb).max(axis=1, keepdims=True), 0.0, rgb)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    zeros = (rgb == 0).sum(axis=1)
    mx = rgb.max(axis=1)
    luma = _luma(rgb)
    lit = mx > 0
    # the peak the Khronos curve looks at: after the offset x - 6.25 x^2 (x = the smallest channel, below 0.08) or 0.04
    x = rgb.min(axis=1)
    peak = mx - np.where(x < 0.08, x - 6.25 * x * x, 0.04)
    stops = np.log2(mx[lit].max() / mx[lit].min()) if lit.any() else 0.0
    return {
        "black": int((zeros == 3).sum()), "two_zero": int((zeros == 2).sum()), "one_zero": int((zeros == 1).sum()),
        "max_r": int(((r > g) & (r > b)).sum()), "max_g": int(((g > r) & (g > b)).sum()), "max_b": int(((b > r) & (b > g)).sum()),
        "max_rg": int(((r == g) & (r > b)).sum()), "max_rb": int(((r == b) & (r > g)).sum()), "max_gb": int(((g == b) & (g > r)).sum()),
        "luma_lt_0.04": int((lit & (luma < 0.04)).sum()), "luma_0.04_0.18": int(((luma >= 0.04) & (luma < 0.18)).sum()),
        "luma_0.18_0.75": int(((luma >= 0.18) & (luma < 0.75)).sum()), "luma_gt_0.75": int((luma >= 0.75).sum()),
        "khronos_below": int((lit & (peak < KHRONOS_START)).sum()), "khronos_above": int((peak >= KHRONOS_START).sum()),
        "stops": float(stops),
    }


# ---- what single precision costs the chain ---------------------------------------------------------------------------------------------------
# own(config) = max over all_cards() (the synthetic cards and the oracle's renders of the device's card) and over all channels of
# own_distance(): post_ref's own code in float32 against itself in float64, both clipped to [0, 1] (display units), and in float64
# against itself on a card raised by one float32 ulp of the contrast pass's eps.  None of the post-process code under test takes part.
#
# The sweep is not uniformly well-conditioned, and where it is not, the reference's own two runs say so.  Three causes account for it:
#   (1) the contrast pass computes exp2(log2(x + 1e-6)) - 1e-6: on a pixel near black the result is the rounding residue of that
#       cancellation, and a grade that lifts the shadows steeply (a midtone grade well above 0.5, a large gain, AgX power < 1) shows it;
#   (2) a degenerate grade: midtone grade <= 0 or >= 1, or lift >= gain, makes 1 / gamma infinite or negative, and the image a step at 1;
#   (3) flim's sigmoid with its toe beyond its shoulder, a density of 0 (every pixel equals both caps: invLerp(x, 1, 1) = 0 / 0), or a
#       print exposure that leaves log2(mono + offset) - log2(offset) with no significant bits.
# Half of the random combinations draw (2), since the midtone offset alone spans -100..100 around a grade of 0.5.
#
# ILL: a configuration with own(config) above it is ill-conditioned.  The RGBA8 rule below needs 2 * 255 * BOUND <= 10 % of a byte step,
# BOUND <= 1.96e-4, PRECISION <= 4.9e-5; ILL = 4e-5 keeps a margin to that.
# PRECISION[tm] = max of own(config) over the well-conditioned configurations of sweep(tm); bound(tm) = 4 x that: the deterministic
# log2 / exp2 polynomials are a few ulp looser than libm, and the product associates differently.
# UNSTABLE names every ill-conditioned configuration with its own(config).  They are compared all the same, pixel by pixel: a pixel is
# held to 4 x max(PRECISION, its own |float32 - float64|), so that only the pixels the reference itself cannot pin are let off.
# EXCUSED: configurations not compared at all, with the reason.
ILL = 4e-5
PRECISION = {
    abi.TONEMAP_NONE: 1.905e-05,   # 63 of 119 configurations are well-conditioned
    abi.TONEMAP_AGX: 3.854e-05,   # 121 of 139 configurations are well-conditioned
    abi.TONEMAP_KHRONOS_PBR: 3.399e-05,   # 80 of 123 configurations are well-conditioned
    abi.TONEMAP_FLIM: 3.746e-05,   # 157 of 187 configurations are well-conditioned
}
UNSTABLE = {   # name: its own |float32 - float64| over all cards
    'none/ca_amount=-100': 0.00048, 'none/ca_amount=100': 0.00042, 'none/saturation=100': 6.9e-05, 'none/midtone_color[0]=1': 0.0082,
    'none/midtone_color[1]=1': 0.0065, 'none/midtone_color[2]=1': 0.0062, 'none/midtone_offset=-100': 1, 'none/midtone_offset=100': 1,
    'none/random00': 0.00031, 'none/random02': 4.7e-05, 'none/random03': 0.0018, 'none/random04': 0.0002, 'none/random05': 0.0012,
    'none/random06': 0.023, 'none/random07': 0.0025, 'none/random08': 0.0014, 'none/random10': 0.0012, 'none/random14': 0.0016, 'none/random15': 1,
    'none/random17': 0.0034, 'none/random19': 0.00081, 'none/random20': 0.34, 'none/random21': 0.12, 'none/random22': 0.00072,
    'none/random24': 0.0033, 'none/random26': 0.00044, 'none/random27': 0.004, 'none/random28': 9.9e-05, 'none/random30': 0.0058,
    'none/random31': 0.00042, 'none/random32': 0.0063, 'none/random33': 5.8e-05, 'none/random34': 0.00024, 'none/random35': 0.0015,
    'none/random36': 0.0031, 'none/random37': 1, 'none/random38': 0.00012, 'none/random40': 0.00024, 'none/random41': 0.0031, 'none/random42': 0.0005,
    'none/random43': 0.0049, 'none/random44': 0.0043, 'none/random46': 0.012, 'none/random47': 0.0058, 'none/random48': 0.00057,
    'none/random49': 0.011, 'none/random50': 0.00031, 'none/random55': 0.0012, 'none/random56': 0.00019, 'none/random57': 0.0038,
    'none/random58': 0.0048, 'none/random59': 0.4, 'none/random60': 0.0009, 'none/random61': 0.00068, 'none/random62': 0.00023,
    'none/random63': 0.00026,
    'agx/ca_amount=-100': 0.00017, 'agx/ca_amount=100': 0.00038, 'agx/shadow_offset=-100': 0.00013, 'agx/agx_power[0]=5': 6.9e-05,
    'agx/agx_saturation=3': 4.8e-05, 'agx/random01': 0.014, 'agx/random08': 0.0016, 'agx/random16': 0.00041, 'agx/random17': 0.0035,
    'agx/random23': 0.008, 'agx/random25': 0.023, 'agx/random42': 0.016, 'agx/random44': 0.0032, 'agx/random45': 0.0033, 'agx/random47': 0.0013,
    'agx/random48': 0.00095, 'agx/random57': 0.22, 'agx/random58': 0.0081,
    'khronos/ca_amount=-100': 0.0004, 'khronos/ca_amount=100': 0.00033, 'khronos/midtone_offset=100': 1, 'khronos/random01': 0.0021,
    'khronos/random02': 1, 'khronos/random03': 0.0049, 'khronos/random04': 0.00023, 'khronos/random05': 0.002, 'khronos/random07': 0.00084,
    'khronos/random09': 0.00023, 'khronos/random11': 0.13, 'khronos/random13': 0.2, 'khronos/random15': 0.0039, 'khronos/random17': 0.0008,
    'khronos/random19': 0.00048, 'khronos/random20': 0.19, 'khronos/random21': 0.00036, 'khronos/random23': 0.0014, 'khronos/random25': 0.0018,
    'khronos/random28': 0.0013, 'khronos/random29': 0.00042, 'khronos/random31': 0.0024, 'khronos/random33': 0.0047, 'khronos/random34': 0.0001,
    'khronos/random35': 0.0008, 'khronos/random36': 0.0015, 'khronos/random37': 0.00043, 'khronos/random38': 0.0024, 'khronos/random39': 0.0068,
    'khronos/random42': 0.24, 'khronos/random43': 0.00071, 'khronos/random44': 1, 'khronos/random45': 0.00065, 'khronos/random47': 0.0046,
    'khronos/random49': 8.7e-05, 'khronos/random50': 0.0024, 'khronos/random51': 0.2, 'khronos/random52': 0.14, 'khronos/random53': 0.0019,
    'khronos/random56': 0.024, 'khronos/random59': 0.00016, 'khronos/random62': 1, 'khronos/random63': 6.1e-05,
    'flim/ca_amount=-100': 0.00036, 'flim/ca_amount=100': 0.0011, 'flim/shadow_color[2]=1': 9.4e-05, 'flim/midtone_color[0]=0': 9e-05,
    'flim/midtone_color[0]=1': 0.029, 'flim/midtone_color[1]=0': 0.00021, 'flim/midtone_color[1]=1': 0.024, 'flim/midtone_color[2]=1': 0.055,
    'flim/midtone_offset=100': 1, 'flim/highlight_offset=100': 0.00051, 'flim/flim_sigmoid_toe[0]=1': 1, 'flim/flim_sigmoid_shoulder[1]=0': 1,
    'flim/flim_negative_density=0': 1, 'flim/flim_print_exposure=-10': 0.1, 'flim/random00': 1, 'flim/random04': 1, 'flim/random06': 1,
    'flim/random08': 1, 'flim/random11': 0.2, 'flim/random14': 1, 'flim/random23': 0.71, 'flim/random25': 0.46, 'flim/random26': 0.002,
    'flim/random30': 1, 'flim/random37': 1, 'flim/random47': 0.22, 'flim/random48': 0.084, 'flim/random49': 0.59, 'flim/random51': 1,
    'flim/random59': 0.0065,
}
EXCUSED = {
    "flim/flim_sigmoid_shoulder[1]=0": "a shoulder below the toe makes the slope negative and the toe's exponent negative: the curve jumps "
                                       "from 0 to +inf at x = 0, and six near-black pixels of the cards sit on either side by one rounding",
    "flim/random48": "the same jump: toe.x 0.65 lies beyond shoulder.x 0.16, and with sigmoid_log2_min 4.4 every dark pixel has mono << offset, so "
                     "x = invLerp(log2(mono + exp2(min)), min, max) is 0 or one rounding above it; the polynomials' log2(exp2(min)) lands above "
                     "min where libm's lands on it (4 pixels of the rendered card)",
    "flim/flim_print_exposure=-10": "cause (3): the print stage sees mono << offset; the oracle's log2 polynomial loses up to 5x what "
                                    "np.log2 loses in float32 there (0.05 against 0.01 per pixel), more than the factor 4 allows",
}


def bound(tm):
    return 4.0 * PRECISION[tm]


EPS_ULP = float(np.spacing(f32(1e-6)))     # 1.1e-13: single precision cannot resolve x + 1e-6, the contrast pass's first step, finer than this


def own_distance(acc, po, to, working_space, d64=None):
    """Per pixel [H, W, 1], on the reference alone: how far single precision moves the display colour.  The larger of
    |float32 run - float64 run| and |float64 run of the card raised by EPS_ULP - float64 run|: on an exactly black pixel numpy's
    exp2(log2(1e-6)) - 1e-6 happens to cancel to 0 in float32 as well, where any other log2 / exp2 leaves a residue of a few EPS_ULP.
    inf where one run is NaN and another is not."""
    if d64 is None:
        d64, _ = post_ref.postprocess(acc, po, to, working_space)
    d32, _ = post_ref.postprocess(acc, po, to, working_space, dtype=np.float32)
    raised = np.array(acc, dtype=np.float64)
    raised[..., :3] += EPS_ULP
    dup, _ = post_ref.postprocess(raised, po, to, working_space)
    a = clipped(d64)
    own = np.zeros(a.shape[:2] + (1,))
    for other in (clipped(d32), clipped(dup)):
        d = np.where(np.isnan(a) != np.isnan(other), np.inf, np.nan_to_num(np.abs(a - other), nan=0.0))
        own = np.maximum(own, d.max(axis=-1, keepdims=True))
    return own


def tolerance(cfg, acc, d64, working_space):
    """The per-channel tolerance [H, W, 1] of `cfg` on `acc`: bound(tm), and for a configuration of UNSTABLE 4 x the pixel's
    own_distance() where that is larger."""
    tol = np.full(d64.shape[:2] + (1,), bound(cfg.tonemapper))
    if cfg.name in UNSTABLE:
        po, to = cfg.structs()
        tol = np.maximum(tol, 4.0 * own_distance(acc, po, to, working_space, d64))
    return tol


def clipped(display):
    """Display colour clipped to [0, 1]; NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.clip(np.asarray(display, dtype=np.float64), 0.0, 1.0)


def all_cards():
    """[(accumulator, working space)]: the synthetic cards, and the oracle's render of the device's card at every size of GPU_SIZES."""
    import oracle_lib
    from platinum_amd.renderer import make_params
    out = [(card(w, h), scenes.colorspace(scenes.BT2020)) for w, h in CARD_SIZES]
    for w, h in GPU_SIZES:
        o = oracle_lib.OracleScene(card_scene(w, h), make_params(w, h, 1, 1, working_space=GPU_WORKING_SPACE))
        out.append((o.render(0, 1), scenes.colorspace(GPU_WORKING_SPACE)))
        o.close()
    return out


def measure_precision(tm, cards=None):
    """{config name: max of own_distance()} for sweep(tm) over `cards` (default: all_cards())."""
    cards = cards if cards is not None else all_cards()
    out = {}
    for cfg in sweep(tm):
        po, to = cfg.structs()
        out[cfg.name] = max(float(own_distance(acc, po, to, ws).max()) for acc, ws in cards)
    return out


# ---- the RGBA8 rule ----------------------------------------------------------------------------------------------------------------------------
def excusable(display, tol):
    """Channels whose byte may differ by 1: 255 * reference lies within 255 * tol of a rounding boundary k + 0.5."""
    x = clipped(display) * 255.0
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.floor(x) - 0.5) <= 255.0 * tol


def rgba8_violations(got, display, tol):
    """Channels [H, W, 3] where the bytes `got` [H, W, 4] break the rule against the reference's display colour; alpha must be 255."""
    want = post_ref.quantise(display)
    diff = np.abs(got[..., :3].astype(np.int32) - want[..., :3].astype(np.int32))
    bad = (diff > 1) | ((diff == 1) & ~excusable(display, tol))
    bad &= np.broadcast_to(np.asarray(tol) <= 0.5 / 255.0, bad.shape)   # (a pixel of an UNSTABLE configuration let off by tolerance())
    bad[..., 0] |= got[..., 3] != 255
    return bad


def card_statistics(display, tol):
    """(share of excusable channel values, share of channel values in 1..254) of a reference image."""
    q = post_ref.quantise(display)[..., :3]
    return float(excusable(display, tol).mean()), float(((q >= 1) & (q <= 254)).mean())


# ---- the GMoN resolve ----------------------------------------------------------------------------------------------------------------------------
# Gini-weighted median of means: per pixel the n bucket means are sorted by luma (a stable bubble sort), the
# Gini coefficient G of the sorted values is taken, c = int(min(G, cap) * (n / 2)) buckets are trimmed from either end (n / 2 an integer
# division) and the rest is averaged.  G is 0 / 0 on an all-black pixel; NaN or a negative product trims nothing.
def _luma32(v):
    return (v[..., 0] * f32(0.2126) + v[..., 1] * f32(0.7152)) + v[..., 2] * f32(0.0722)


def gmon_resolve(buckets, cap):
    """float32, in the kernel's order of operations, a loop over buckets and vectorised over pixels: buckets [n, H, W, 4] -> [H, W, 4]."""
    n = len(buckets)
    v = [np.array(b[..., :3], dtype=f32) for b in buckets]
    with np.errstate(all="ignore"):
        for i in range(n, 1, -1):
            for j in range(1, i):
                swap = (_luma32(v[j]) < _luma32(v[j - 1]))[..., None]
                v[j - 1], v[j] = np.where(swap, v[j], v[j - 1]), np.where(swap, v[j - 1], v[j])
        total, weighted = np.zeros_like(v[0]), np.zeros_like(v[0])
        for i in range(n):
            total = total + v[i]
            weighted = weighted + f32(i + 1) * v[i]
        G = (f32(2) * _luma32(weighted)) / (f32(n) * _luma32(total)) - f32(n + 1) / f32(n)
        G = np.fmin(G, f32(cap))
        cf = G * f32(n // 2)
        c = np.where(cf > 0, np.nan_to_num(cf, nan=0.0, posinf=0.0), 0).astype(np.int32)
        kept = np.zeros_like(v[0])
        for i in range(n):
            inside = ((i >= c) & (i < n - c))[..., None]
            kept = np.where(inside, kept + v[i], kept)
        color = kept / (f32(n) - f32(2) * c.astype(f32))[..., None]
    out = np.ones(color.shape[:2] + (4,), dtype=f32)
    out[..., :3] = color
    return out


def gmon_quantities(buckets, cap, dtype=np.float64):
    """The same quantities from their definitions, in `dtype`: (G [H, W], trimmed mean [H, W, 3], c [H, W], G * (n // 2) [H, W]).
    G is the Gini coefficient of the bucket lumas, sum_ij |l_i - l_j| / (2 n sum_i l_i); the trimmed mean drops the c darkest and the
    c brightest buckets."""
    b = np.asarray(buckets)[..., :3].astype(dtype)
    n = len(b)
    luma = (b * np.array([0.2126, 0.7152, 0.0722], dtype=dtype)).sum(axis=-1)                      # [n, H, W]
    with np.errstate(all="ignore"):
        G = np.abs(luma[:, None] - luma[None, :]).sum(axis=(0, 1)) / (dtype(2 * n) * luma.sum(axis=0))
        cf = np.fmin(G, dtype(cap)) * dtype(n // 2)
        c = np.where(cf > 0, cf, 0).astype(np.int64)
        order = np.argsort(luma, axis=0, kind="stable")
        ranked = np.take_along_axis(b, order[..., None], axis=0)
        rank = np.arange(n)[:, None, None]
        keep = ((rank >= c[None]) & (rank < n - c[None]))[..., None]
        mean = (ranked * keep).sum(axis=0) / (n - 2 * c)[..., None].astype(dtype)
    return G, mean, c, cf


# ---- a test card for the device --------------------------------------------------------------------------------------------------------------
# No entry uploads an accumulator, so the device renders its card: a grid of emissive quads (black base colour, one emission colour and
# strength each) that fills the frame exactly, seen head-on at the focus distance by a far camera, 1 spp, max_bounces = 1.  One patch is
# left out: the background there is exact black.  The accumulator read back from the device is what device, oracle and reference post-process.
GRID = (8, 8)
GPU_WORKING_SPACE = scenes.BT709     # the materials' own space: the renderer's input transform leaves the patch colours (all but) untouched
GPU_SIZES = [(17, 15), (16, 16), (257, 1), (1, 1), (96, 64), (64, 96)]     # W * H one below, at and one above kBlock = 256; portrait last
CAMERA_DISTANCE = 100.0


def patch_colours():
    """GRID[0] * GRID[1] - 1 emission colours: two of every block of special_pixels() but the black one, the rest log-uniform."""
    special = np.concatenate([v[:2] for k, v in special_pixels().items() if k != "black"])
    n = GRID[0] * GRID[1] - 1 - len(special)
    rng = np.random.default_rng(77)
    level = MID_GREY * np.exp2(rng.uniform(-STOPS / 2, STOPS / 2, size=n))
    chroma = rng.uniform(0.05, 1.0, size=(n, 3))
    chroma /= chroma.max(axis=1, keepdims=True)
    colours = np.concatenate([special, (level[:, None] * chroma).astype(f32)])
    return colours[np.random.default_rng(78).permutation(len(colours))]


def card_scene(w, h):
    """The patch grid sized to the view of a w x h image."""
    cam = scenes.Camera(sensor_size=(36.0, 24.0), focal_length=50.0, focus_distance=CAMERA_DISTANCE)
    aspect = w / h
    view_h = CAMERA_DISTANCE * (36.0 / max(36.0 / 24.0, aspect)) / 50.0          # the view rectangle at the focus distance
    view_w = view_h * aspect
    sc = scenes.Scene(name="post_card_%dx%d" % (w, h))
    quad = sc.add_mesh(scenes.plane(1.0))
    gx, gy = GRID
    sx, sz = view_w / gx, view_h / gy
    colours = patch_colours()
    k = 0
    for j in range(gy):
        for i in range(gx):
            if (i, j) == (gx // 2, gy // 2):
                continue                                                          # the patch left out
            c = colours[k]
            k += 1
            strength = float(c.max())
            mat = scenes.Material(name="patch%d" % k, base_color=(0.0, 0.0, 0.0, 1.0), emission=tuple(float(v) for v in c / c.max()),
                                  emission_strength=strength)
            x, z = (i + 0.5) * sx - view_w / 2, (j + 0.5) * sz - view_h / 2
            sc.add_instance(quad, scenes.Transform(translation=(x, 0.0, z), scale=(sx, 1.0, sz)), [mat])
    sc.set_camera(cam, scenes.Transform(translation=(0.0, CAMERA_DISTANCE, 0.0), target=(0.0, 0.0, 0.0), track=True))
    return sc
