"""An independent restatement of the post-process chain and tonemap pass — TEST INFRASTRUCTURE, plain numpy.

Written from the formulas the chain is defined by (the passes of the reference's postprocess.metal in the order of
renderer_pt.cpp:343-353, the option structs of postprocessing.hpp, the colour-space transform of colorspace.cpp), not from pt_post.h or
oracle/post_oracle.inc: it is vectorised over the image, computes in float64, uses np.log2 / np.exp2 / np.power instead of the
deterministic polynomials, and derives the output transform itself from the chromaticities.  `postprocess(..., dtype=np.float32)` runs
the very same code with every array in single precision: the distance between the two runs is what single precision costs this chain
(post_lib.PRECISION), measured without any of the code under test.

Conventions where MSL leaves the result undefined — the project's choice, followed here:
  * powr(x, y) with x <= 0 is 0 (MSL: undefined for x < 0).  AgX's look uses the same rule for its pow.  This decides AgX's darkest channels.
    Elsewhere powr(x, y) is exp2(y * log2(x)) in its edge cases as well: powr(1, +-inf) and powr(+inf, 0) are NaN (0 * inf), unlike pow.
    A midtone grade at or below zero makes 1 / gamma infinite and meets that case at every channel that is exactly 1.
  * saturate(NaN) is 0, and the RGBA8 store writes NaN as 0.  min / max return the operand that is not NaN.
  * log2 / log10 of a value that is not > 0 is -inf.
  * flim's uniform offset multiplies by mono2 / mono, 0 / 0 on a black pixel: the NaN meets the saturate that follows and ends as 0.
  * exp2 and powr overflow to +inf and underflow to 0, as IEEE arithmetic does.
  * The contrast pass hands on at most 2^64 per channel.  An overbright pixel is thereby "far above white" and finite: +inf would turn
    the blends after it (inf - inf, 0 * inf) into NaN, and NaN into black.
"""
import numpy as np

LW = (0.2126, 0.7152, 0.0722)                       # luma weights
CEILING = 2.0 ** 64
TONEMAP_NONE, TONEMAP_AGX, TONEMAP_KHRONOS_PBR, TONEMAP_FLIM = 0, 1, 2, 3
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def options(struct):
    """A ctypes option struct as {field: float | tuple | dict}, nested structs included."""
    out = {}
    for name, _t in struct._fields_:
        v = getattr(struct, name)
        if hasattr(v, "_fields_"):
            out[name] = options(v)
        elif hasattr(v, "__len__"):
            out[name] = tuple(v)
        else:
            out[name] = v
    return out


def colorspace_to_xyz(cs, F=np.float64):
    """RGB -> XYZ of a colour space given as {r, g, b, w: (x, y)} chromaticities (Y of the white point = 1)."""
    def xyz(p):
        return np.array([p[0], p[1], 1.0 - p[0] - p[1]], dtype=F)
    prim = np.stack([xyz(cs["r"]), xyz(cs["g"]), xyz(cs["b"])], axis=1)     # primaries as columns
    w = xyz(cs["w"])
    white = w / w[1]
    scale = np.linalg.inv(prim) @ white                                     # white = prim @ diag(scale) @ (1, 1, 1)
    return (prim * scale[None, :]).astype(F)


def output_transform(working, output, F=np.float64):
    """The matrix that takes working-space RGB to output-space RGB: fromXYZ(output) @ toXYZ(working)."""
    return (np.linalg.inv(colorspace_to_xyz(output, F)) @ colorspace_to_xyz(working, F)).astype(F)


class _Chain:
    def __init__(self, F):
        self.F = F
        self.lw = np.array(LW, dtype=F)

    # ---- scalar helpers, all elementwise ------------------------------------------------------------------------------------
    def c(self, v):
        return self.F(v)

    def vec(self, v):
        return np.array(v, dtype=self.F)

    def saturate(self, x):
        x = np.asarray(x, dtype=self.F)
        return np.where(x > 0, np.minimum(x, self.c(1)), self.c(0)).astype(self.F)

    def log(self, x, fn=np.log2):
        x = np.asarray(x, dtype=self.F)
        return np.where(x > 0, fn(np.where(x > 0, x, self.c(1))), self.c(-np.inf)).astype(self.F)

    def powr(self, x, y):
        x, y = np.asarray(x, dtype=self.F), np.asarray(y, dtype=self.F)
        base = np.where(x <= 0, self.c(1), x)
        # powr, not pow: where y * log2(x) is 0 * inf the result is NaN (powr(1, inf), powr(inf, 0)), not pow's 1
        r = np.where(np.isnan(y * np.log2(base)), self.c(np.nan), np.power(base, y))
        return np.where(x <= 0, self.c(0), r).astype(self.F)

    def exp2(self, x):
        return np.exp2(np.asarray(x, dtype=self.F)).astype(self.F)

    def mix(self, a, b, t):
        return a + (b - a) * t

    def inv_lerp(self, x, s, e):
        return self.saturate((x - s) / (e - s))

    def smoothstep(self, e0, e1, x):
        t = self.saturate((x - self.c(e0)) / (self.c(e1) - self.c(e0)))
        return t * t * (self.c(3) - self.c(2) * t)

    def luma(self, rgb):
        return rgb[..., 0] * self.lw[0] + rgb[..., 1] * self.lw[1] + rgb[..., 2] * self.lw[2]

    def avg(self, rgb):
        return (rgb[..., 0] + rgb[..., 1] + rgb[..., 2]) / self.c(3)

    def mat_vec(self, cols, v):
        """M @ v for M given by its three columns."""
        return cols[0] * v[..., 0:1] + cols[1] * v[..., 1:2] + cols[2] * v[..., 2:3]

    # ---- AgX ------------------------------------------------------------------------------------------------------------------
    AGX_IN = ((0.842479062253094, 0.0423282422610123, 0.0423756549057051),
              (0.0784335999999992, 0.878468636469772, 0.0784336),
              (0.0792237451477643, 0.0791661274605434, 0.879142973793104))
    AGX_OUT = ((1.19687900512017, -0.0528968517574562, -0.0529716355144438),
               (-0.0980208811401368, 1.15190312990417, -0.0980434501171241),
               (-0.0990297440797205, -0.0989611768448433, 1.15107367264116))
    AGX_MIN_EV, AGX_MAX_EV = -12.47393, 4.026069

    def agx(self, val, o):
        c = self.c
        lo, hi = c(self.AGX_MIN_EV), c(self.AGX_MAX_EV)
        val = self.mat_vec(self.vec(self.AGX_IN), val)
        val = np.clip(self.log(val), lo, hi)
        x = (val - lo) / (hi - lo)
        x2 = x * x
        x4 = x2 * x2
        val = (c(15.5) * x4 * x2 - c(40.14) * x4 * x + c(31.96) * x4 - c(6.868) * x2 * x + c(0.4298) * x2 + c(0.1191) * x - c(0.00232))
        luma = self.luma(val)[..., None]                                            # the look
        look = self.powr(val * self.vec(o["agx_slope"]) + self.vec(o["agx_offset"]), self.vec(o["agx_power"]))
        val = self.mix(luma, look, c(o["agx_saturation"]))
        val = self.saturate(self.mat_vec(self.vec(self.AGX_OUT), val))
        return self.powr(val, c(2.2))                                               # linearise the AgX output

    # ---- Khronos PBR neutral ---------------------------------------------------------------------------------------------------
    def khronos(self, val, o):
        c = self.c
        start = c(o["khr_compression_start"]) - c(0.04)
        x = np.fmin(val[..., 0], np.fmin(val[..., 1], val[..., 2]))
        offset = np.where(x < c(0.08), x - c(6.25) * x * x, c(0.04))
        val = val - offset[..., None]
        peak = np.fmax(val[..., 0], np.fmax(val[..., 1], val[..., 2]))
        d = c(1) - start
        new_peak = c(1) - d * d / (peak + d - start)
        scaled = val * (new_peak / peak)[..., None]
        g = c(1) - c(1) / (c(o["khr_desaturation"]) * (peak - new_peak) + c(1))
        out = self.mix(scaled, new_peak[..., None], g[..., None])
        return np.where((peak < start)[..., None], val, out)

    # ---- flim --------------------------------------------------------------------------------------------------------------------
    def rgb_to_hsv(self, rgb):
        c = self.c
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        cmax = np.fmax(np.fmax(r, g), b)
        cmin = np.fmin(np.fmin(r, g), b)
        delta = cmax - cmin
        s = np.where(cmax != 0, delta / cmax, c(0))
        cr, cg, cb = (cmax - r) / delta, (cmax - g) / delta, (cmax - b) / delta
        h = np.where(r == cmax, cb - cg, np.where(g == cmax, c(2) + cr - cb, c(4) + cg - cr)) / c(6)
        h = np.where(h < 0, h + c(1), h)
        return np.where(s != 0, h, c(0)), s, cmax

    def hsv_to_rgb(self, h, s, v):
        c = self.c
        h = np.where(h == 1, c(0), h) * c(6)
        i = np.floor(h)
        f = h - i
        p, q, t = v * (c(1) - s), v * (c(1) - s * f), v * (c(1) - s * (c(1) - f))
        sextants = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v)]
        out = []
        for ch in range(3):
            col = (v, p, q)[ch] + np.zeros_like(h)
            for k, sx in enumerate(sextants):
                col = np.where(i == k, sx[ch], col)
            out.append(np.where(s == 0, v, col))
        return np.stack(np.broadcast_arrays(*out), axis=-1).astype(self.F)

    def hue_sat(self, color, hue, sat, value):
        h, s, v = self.rgb_to_hsv(color)
        h = h + self.c(hue) + self.c(0.5)
        h = h - np.floor(h)
        return self.hsv_to_rgb(h, self.saturate(s * sat), v * self.c(value))

    def gamut_row(self, hue, scale, rotate, mul):
        c = self.c
        h = np.fmod(c(hue) + c(rotate) / c(360), c(1))
        row = self.hsv_to_rgb(np.asarray(h, dtype=self.F), np.asarray(c(1) / c(scale)), np.asarray(c(1)))
        return row / (row[0] + row[1] + row[2]) * c(mul)

    def super_sigmoid(self, x, toe, shoulder):
        c = self.c
        x = self.saturate(x)
        tx, ty = self.saturate(toe[0]), self.saturate(toe[1])
        sx, sy = self.saturate(shoulder[0]), self.saturate(shoulder[1])
        slope = (sy - ty) / (sx - tx)
        toe_v = ty * self.powr(x / tx, slope * tx / ty)
        line = slope * x + ty - slope * tx
        sh_pow = -slope / ((sx - c(1)) / self.powr(c(1) - sx, c(2)) * (c(1) - sy))
        sh_v = (c(1) - self.powr(c(1) - (x - sx) / (c(1) - sx), sh_pow)) * (c(1) - sy) + sy
        return np.where(x < tx, toe_v, np.where(x < sx, line, sh_v))

    def dye_mix_factor(self, mono, max_density, o):
        c = self.c
        lo, hi = c(o["flim_sigmoid_log2_min"]), c(o["flim_sigmoid_log2_max"])
        fac = self.inv_lerp(self.log(mono + self.exp2(lo)), lo, hi)
        fac = self.super_sigmoid(fac, self.vec(o["flim_sigmoid_toe"]), self.vec(o["flim_sigmoid_shoulder"]))
        return self.saturate(self.exp2(-(fac * c(max_density))))

    def develop(self, color, exposure, max_density, o):
        color = color * self.exp2(self.c(exposure))
        result = None
        for sens_ch, dye in ((2, (1, 1, 0)), (1, (1, 0, 1)), (0, (0, 1, 1))):     # blue-, green-, red-sensitive layer
            mono = color[..., sens_ch]                                              # the sensitivity tones are unit vectors: dot() picks a channel
            fac = self.dye_mix_factor(mono, max_density, o)[..., None]
            layer = self.mix(self.vec(dye), self.c(1), fac)
            result = layer if result is None else result * layer
        return result

    def negative_and_print(self, color, backlight, o):
        color = self.develop(color, o["flim_negative_exposure"], o["flim_negative_density"], o)
        return self.develop(color * backlight, o["flim_print_exposure"], o["flim_print_density"], o)

    def uniform_offset(self, color, black_point, white_point):
        mono = self.avg(color)
        mono2 = self.inv_lerp(mono, black_point / self.c(1000), self.c(1) - white_point / self.c(1000))
        return color * (mono2 / mono)[..., None]

    def flim(self, val, o):
        c = self.c
        val = val * self.exp2(c(o["flim_pre_exposure"]))
        sc, rot, mul = o["flim_extended_gamut_scale"], o["flim_extended_gamut_rotation"], o["flim_extended_gamut_mul"]
        # the extension matrix holds one gamut row per primary as a COLUMN; colours multiply it from the left (row vector times matrix)
        ext = np.stack([self.gamut_row(k / 3.0, sc[k], rot[k], mul[k]) for k in range(3)], axis=1).astype(self.F)
        ext_inv = np.linalg.inv(ext).astype(self.F)
        backlight = self.vec(o["flim_print_backlight"]) @ ext
        white_cap = self.negative_and_print(np.full(3, 1e7, dtype=self.F), backlight, o)
        val = self.mix(val, val * self.vec(o["flim_pre_formation_filter"]), c(o["flim_pre_formation_filter_strength"]))
        val = val @ ext
        val = self.negative_and_print(val, backlight, o)
        val = val @ ext_inv
        val = np.fmax(val, c(0)) / white_cap
        if o["flim_auto_black_point"]:
            black_cap = self.negative_and_print(np.zeros(3, dtype=self.F), backlight, o) / white_cap
            val = self.uniform_offset(val, self.avg(black_cap) * c(1000), c(0))
        else:
            val = self.uniform_offset(val, c(o["flim_black_point"]), c(0))
        val = self.mix(val, val * self.vec(o["flim_post_formation_filter"]), c(o["flim_post_formation_filter_strength"]))
        val = self.saturate(val)
        mono = self.avg(val)
        fac = np.where(mono < c(0.5), self.inv_lerp(mono, c(0.05), c(0.5)), self.inv_lerp(mono, c(0.95), c(0.5)))
        val = self.mix(val, self.hue_sat(val, 0.5, c(o["flim_midtone_saturation"]), 1.0), fac[..., None])
        return self.saturate(val)

    def flim_white_cap(self, o):
        """The colour flim gives a pixel at the contrast pass's ceiling, before lift / gamma / gain: both develop stages saturated, as
        for the 1e7 its white cap is defined with, then the black point, the post-formation filter and the midtone saturation."""
        return self.flim(np.full((1, 1, 3), CEILING, dtype=self.F), o)

    # ---- spatial passes ------------------------------------------------------------------------------------------------------------
    def aspect_uv(self, u, v, aspect, inverse=False):
        c = self.c
        if aspect > 1:
            v = (v - c(0.5)) * aspect + c(0.5) if inverse else (v - c(0.5)) / aspect + c(0.5)
        else:
            u = (u - c(0.5)) / aspect + c(0.5) if inverse else (u - c(0.5)) * aspect + c(0.5)
        return u, v

    def bilinear(self, img, u, v):
        """Linear filtering with clamp-to-edge addressing of one channel image at normalised coordinates."""
        c = self.c
        H, W = img.shape
        x, y = u * c(W) - c(0.5), v * c(H) - c(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        xi0, yi0 = np.clip(x0.astype(np.int64), 0, W - 1), np.clip(y0.astype(np.int64), 0, H - 1)
        xi1, yi1 = np.clip(x0.astype(np.int64) + 1, 0, W - 1), np.clip(y0.astype(np.int64) + 1, 0, H - 1)
        top = self.mix(img[yi0, xi0], img[yi0, xi1], fx)
        bot = self.mix(img[yi1, xi0], img[yi1, xi1], fx)
        return self.mix(top, bot, fy)

    def run(self, acc, post, tm, working_space):
        F, c = self.F, self.c
        H, W = acc.shape[:2]
        u = np.broadcast_to(((np.arange(W, dtype=F) + c(0.5)) / c(W))[None, :], (H, W))
        v = np.broadcast_to(((np.arange(H, dtype=F) + c(0.5)) / c(H))[:, None], (H, W))
        aspect_img = c(W) / c(H)

        color = acc[..., :3].astype(F) * self.exp2(c(post["exposure"]))                               # exposure

        if post["ca_amount"] != 0.0:                                                                  # lateral chromatic aberration
            um, vm = self.aspect_uv(u, v, aspect_img)
            amount = c(post["ca_amount"]) * c(0.005) * c(0.01)
            scales = (c(1) + amount, c(1) - amount * c(post["ca_green_shift"]) * c(0.01), c(1) - amount)
            chans = []
            for ch, s in enumerate(scales):
                uu, vv = self.aspect_uv((um - c(0.5)) * s + c(0.5), (vm - c(0.5)) * s + c(0.5), aspect_img, inverse=True)
                chans.append(self.bilinear(color[..., ch], uu, vv))
            color = np.stack(chans, axis=-1)

        eps = c(1e-6)                                                                                 # contrast about log2 0.18, saturation
        adj = self.mix(c(0.18), self.log(color + eps), c(1) + c(post["contrast"]) * c(0.01))
        color = np.fmin(np.fmax(c(0), self.exp2(adj) - eps), c(CEILING))
        color = self.mix(self.luma(color)[..., None], color, c(1) + c(post["saturation"]) * c(0.01))

        luma = self.luma(color)                                                                       # tone curve
        for amount, (e0, e1) in ((post["blacks"], (0.04, 0.0)), (post["shadows"], (0.18, 0.0)),
                                 (post["highlights"], (0.18, 1.0)), (post["whites"], (0.75, 1.0))):
            color = color * self.exp2(c(0.01) * c(amount) * self.smoothstep(e0, e1, luma))[..., None]

        aspect = self.mix(c(1), aspect_img, c(post["vig_roundness"]) * c(0.01))                       # vignette
        um, vm = self.aspect_uv(u, v, aspect)
        dist = np.sqrt((um - c(0.5)) ** 2 + (vm - c(0.5)) ** 2) / np.sqrt(c(0.5))
        end = c(1) - c(post["vig_midpoint"]) * c(0.01)
        start = end * (c(1) - c(post["vig_feather"]) * c(0.01))
        d = self.inv_lerp(dist, start, end)
        vig = np.where(d == 0, c(0), self.powr(d, c(post["vig_power"]) * c(0.05))) * self.smoothstep(start, end, dist)
        color = color * self.exp2(c(post["vig_amount"]) * vig)[..., None]

        if tm["tonemapper"] == TONEMAP_AGX:                                                           # tonemap
            color = self.agx(color, tm)
        elif tm["tonemapper"] == TONEMAP_KHRONOS_PBR:
            color = self.khronos(color, tm)
        elif tm["tonemapper"] == TONEMAP_FLIM:
            color = self.flim(color, tm)

        return self.grade_and_encode(color, tm, working_space)

    def grade_and_encode(self, color, tm, working_space):
        """Lift / gamma / gain, the output transform and the sRGB curve: the tonemap pass after the tonemapper."""
        F, c = self.F, self.c
        def centred(col):                                                                             # lift / gamma / gain
            col = self.vec(col)
            return col - self.avg(col)
        lift = centred(tm["shadow_color"]) + c(tm["shadow_offset"]) * c(0.01)
        gain = c(1) + centred(tm["highlight_color"]) + c(tm["highlight_offset"]) * c(0.01)
        mid_gray = c(0.5) + centred(tm["midtone_color"]) + c(tm["midtone_offset"]) * c(0.01)
        gamma = self.log((c(0.5) - lift) / (gain - lift), np.log10) / self.log(mid_gray, np.log10)
        color = self.mix(lift, gain, self.saturate(self.powr(color, c(1) / gamma)))

        odt = output_transform(working_space, tm["output_space"], F)                                  # output transform, sRGB curve
        color = color @ odt.T
        return np.where(color < c(0.0031308), c(12.92) * color, c(1.055) * self.powr(color, c(1) / c(2.4)) - c(0.055)).astype(F)



def quantise(display):
    """The RGBA8Unorm store: clamp to [0, 1], scale by 255, round to nearest; NaN is 0; alpha is 255."""
    d = np.asarray(display)
    with np.errstate(invalid="ignore"):
        q = np.where(d > 0, np.where(d >= 1, 255.0, np.floor(np.where(d > 0, np.minimum(d, 1.0), 0.0) * 255.0 + 0.5)), 0.0)
    out = np.full(d.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = q.astype(np.uint8)
    return out


def postprocess(acc, post, tonemap, working_space, dtype=np.float64):
    """(display colour before quantisation [H, W, 3] in `dtype`, RGBA8 [H, W, 4]) of the accumulator `acc` [H, W, >=3].
    `post`, `tonemap` and `working_space` are ctypes structs (pt_post_options, pt_tonemap_options, pt_colorspace) or options() of them."""
    post, tonemap, working_space = [o if isinstance(o, dict) else options(o) for o in (post, tonemap, working_space)]
    with np.errstate(**_ERR):
        display = _Chain(dtype).run(np.asarray(acc), post, tonemap, working_space)
    return display, quantise(display)


def flim_white_cap(tonemap, dtype=np.float64):
    tonemap = tonemap if isinstance(tonemap, dict) else options(tonemap)
    with np.errstate(**_ERR):
        return _Chain(dtype).flim_white_cap(tonemap)[0, 0]
