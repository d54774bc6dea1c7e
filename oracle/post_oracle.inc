// TEST INFRASTRUCTURE — included by pt_oracle.cpp.  CPU restatement of the reference's post-process chain and tonemap
// pass (src/renderer_pt/shaders/postprocess.metal; options src/core/postprocessing.hpp; pass order
// renderer_pt.cpp:343-353; odt renderer_pt.cpp:190-191).  Each fragment function keeps its name.
namespace post {

const float3 lw = {0.2126f, 0.7152f, 0.0722f};                                       // postprocess.metal:19
inline float luma(float3 c) { return dot(c, lw); }
inline float rgbSum(float3 c) { return c.x + c.y + c.z; }                            // :68-70
inline float rgbAvg(float3 c) { return (c.x + c.y + c.z) / 3.0f; }                   // :72-74
inline float rgbMax(float3 c) { return fmaxf(fmaxf(c.x, c.y), c.z); }                // :76-78
inline float rgbMin(float3 c) { return fminf(fminf(c.x, c.y), c.z); }                // :80-82
inline float invLerp(float x, float s, float e) { return saturate((x - s) / (e - s)); }  // :84-86
inline float smoothstep(float e0, float e1, float x) { float t = saturate((x - e0) / (e1 - e0)); return t * t * (3.0f - 2.0f * t); }
inline float3 mix3(float3 a, float3 b, float t) { return a + (b - a) * t; }
inline float log2s(float x) { return x > 0.0f ? log2_det(x) : -std::numeric_limits<float>::infinity(); }
inline float3 log2v(float3 v) { return {log2s(v.x), log2s(v.y), log2s(v.z)}; }
inline float exp2s(float x) { return x < -125.0f ? 0.0f : (x > 125.0f ? std::numeric_limits<float>::infinity() : exp2_det(x)); }
// exp2_det / powr_det over the whole float range (+inf above, 0 below; in-range arguments unchanged), like pt_post.h's pp_exp2 / pp_powr
inline float exp2g(float x) { return x >= 128.0f ? std::numeric_limits<float>::infinity() : (x < -127.0f ? 0.0f : exp2_det(x)); }
inline float powrg(float x, float y) { return x <= 0.0f ? 0.0f : exp2g(y * log2_det(x)); }
const float ceiling = 18446744073709551616.0f;  // 2^64: what the contrast pass hands on is capped there (pt_post.h kPostCeiling), so that overbright is white, not NaN
inline float3 exp2v(float3 v) { return {exp2g(v.x), exp2g(v.y), exp2g(v.z)}; }
inline float3 sat3(float3 v) { return {saturate(v.x), saturate(v.y), saturate(v.z)}; }
inline float3 vmul(float3 v, const Mat3& m) { return {dot(v, m.c0), dot(v, m.c1), dot(v, m.c2)}; }  // v * M

inline float el(const Mat3& m, int c, int r) { const float3& col = c == 0 ? m.c0 : (c == 1 ? m.c1 : m.c2); return r == 0 ? col.x : (r == 1 ? col.y : col.z); }
Mat3 inverse(const Mat3& m) {  // :42-63
  float a = el(m, 1, 1) * el(m, 2, 2) - el(m, 2, 1) * el(m, 1, 2);
  float b = el(m, 1, 2) * el(m, 2, 0) - el(m, 1, 0) * el(m, 2, 2);
  float c = el(m, 1, 0) * el(m, 2, 1) - el(m, 1, 1) * el(m, 2, 0);
  float det = (el(m, 0, 0) * a + el(m, 0, 1) * b) + el(m, 0, 2) * c;
  float invdet = 1.0f / det;
  Mat3 inv;
  inv.c0 = f3(a * invdet, (el(m, 0, 2) * el(m, 2, 1) - el(m, 0, 1) * el(m, 2, 2)) * invdet, (el(m, 0, 1) * el(m, 1, 2) - el(m, 0, 2) * el(m, 1, 1)) * invdet);
  inv.c1 = f3(b * invdet, (el(m, 0, 0) * el(m, 2, 2) - el(m, 0, 2) * el(m, 2, 0)) * invdet, (el(m, 1, 0) * el(m, 0, 2) - el(m, 0, 0) * el(m, 1, 2)) * invdet);
  inv.c2 = f3(c * invdet, (el(m, 2, 0) * el(m, 0, 1) - el(m, 0, 0) * el(m, 2, 1)) * invdet, (el(m, 0, 0) * el(m, 1, 1) - el(m, 1, 0) * el(m, 0, 1)) * invdet);
  return inv;
}

namespace agx {  // :89-147
float3 contrast(float3 x) {
  float3 x2 = x * x, x4 = x2 * x2;
  return (((((15.5f * x4 * x2 - 40.14f * x4 * x) + 31.96f * x4) - 6.868f * x2 * x) + 0.4298f * x2) + 0.1191f * x) - f3(0.00232f);
}
float3 start(float3 val) {
  const Mat3 M = {f3(0.842479062253094f, 0.0423282422610123f, 0.0423756549057051f), f3(0.0784335999999992f, 0.878468636469772f, 0.0784336f),
                  f3(0.0792237451477643f, 0.0791661274605434f, 0.879142973793104f)};
  const float minEv = -12.47393f, maxEv = 4.026069f;
  val = mul(M, val);
  float3 l = log2v(val);
  val = f3(fminf(fmaxf(l.x, minEv), maxEv), fminf(fmaxf(l.y, minEv), maxEv), fminf(fmaxf(l.z, minEv), maxEv));
  val = (val - f3(minEv)) / (maxEv - minEv);
  return contrast(val);
}
float3 end(float3 val) {
  const Mat3 Mi = {f3(1.19687900512017f, -0.0528968517574562f, -0.0529716355144438f), f3(-0.0980208811401368f, 1.15190312990417f, -0.0980434501171241f),
                   f3(-0.0990297440797205f, -0.0989611768448433f, 1.15107367264116f)};
  return sat3(mul(Mi, val));
}
float3 apply(float3 val, const pt_tonemap_options& o) {
  val = start(val);
  float l = luma(val);
  float3 t = val * f3(o.agx_slope[0], o.agx_slope[1], o.agx_slope[2]) + f3(o.agx_offset[0], o.agx_offset[1], o.agx_offset[2]);
  t = f3(powrg(t.x, o.agx_power[0]), powrg(t.y, o.agx_power[1]), powrg(t.z, o.agx_power[2]));
  val = mix3(f3(l), t, o.agx_saturation);
  return end(val);
}
}  // namespace agx

float3 khronos_apply(float3 val, const pt_tonemap_options& o) {  // :155-175
  float compressionStart = o.khr_compression_start - 0.04f;
  float x = fminf(val.x, fminf(val.y, val.z));
  float offset = x < 0.08f ? x - 6.25f * x * x : 0.04f;
  val = val - f3(offset);
  float peak = fmaxf(val.x, fmaxf(val.y, val.z));
  if (peak < compressionStart) return val;
  float d = 1.0f - compressionStart;
  float newPeak = 1.0f - d * d / (peak + d - compressionStart);
  val *= newPeak / peak;
  float g = 1.0f - 1.0f / (o.khr_desaturation * (peak - newPeak) + 1.0f);
  return mix3(val, f3(newPeak), g);
}

namespace flim {  // :181-413
float wrap(float x, float s, float e) { return s + fmodf(x - s, e - s); }
float3 rgbUniformOffset(float3 color, float blackPoint, float whitePoint) {
  float mono = rgbAvg(color);
  float mono2 = invLerp(mono, blackPoint / 1000.0f, 1.0f - whitePoint / 1000.0f);
  return color * (mono2 / mono);
}
float3 rgbToHsv(float3 rgb) {
  float cmax = rgbMax(rgb), cmin = rgbMin(rgb), cdelta = cmax - cmin;
  float h = 0.0f, s, v = cmax;
  if (cmax != 0.0f) s = cdelta / cmax; else s = 0.0f;
  if (s != 0.0f) {
    float3 c = (f3(cmax) - rgb) / cdelta;
    if (rgb.x == cmax) h = c.z - c.y;
    else if (rgb.y == cmax) h = 2.0f + c.x - c.z;
    else h = 4.0f + c.y - c.x;
    h /= 6.0f;
    if (h < 0.0f) h += 1.0f;
  }
  return f3(h, s, v);
}
float3 hsvToRgb(float3 hsv) {
  float h = hsv.x, s = hsv.y, v = hsv.z;
  if (s == 0.0f) return f3(v);
  if (h == 1.0f) h = 0.0f;
  h *= 6.0f;
  int i = (int)floorf(h);
  float f = h - (float)i;
  float p = v * (1.0f - s), q = v * (1.0f - (s * f)), t = v * (1.0f - (s * (1.0f - f)));
  switch (i) {
    case 0: return f3(v, t, p);
    case 1: return f3(q, v, p);
    case 2: return f3(p, v, t);
    case 3: return f3(p, q, v);
    case 4: return f3(t, p, v);
    default: return f3(v, p, q);
  }
}
float3 hueSat(float3 color, float hue, float sat, float value) {
  float3 hsv = rgbToHsv(color);
  float hh = hsv.x + hue + 0.5f;
  hsv.x = hh - floorf(hh);
  hsv.y = saturate(hsv.y * sat);
  hsv.z *= value;
  return hsvToRgb(hsv);
}
float3 gamutRow(float primaryHue, float scale, float rotate, float mulv) {
  float3 r = hsvToRgb(f3(wrap(primaryHue + (rotate / 360.0f), 0.0f, 1.0f), 1.0f / scale, 1.0f));
  r = r / rgbSum(r);
  return r * mulv;
}
float superSigmoid(float x, float2 toe, float2 shoulder) {
  x = saturate(x);
  toe = {saturate(toe.x), saturate(toe.y)};
  shoulder = {saturate(shoulder.x), saturate(shoulder.y)};
  float slope = (shoulder.y - toe.y) / (shoulder.x - toe.x);
  if (x < toe.x) return toe.y * powrg(x / toe.x, slope * toe.x / toe.y);
  if (x < shoulder.x) return slope * x + toe.y - (slope * toe.x);
  float shoulderPow = -slope / ((shoulder.x - 1.0f) / powrg(1.0f - shoulder.x, 2.0f) * (1.0f - shoulder.y));
  return (1.0f - powrg(1.0f - (x - shoulder.x) / (1.0f - shoulder.x), shoulderPow)) * (1.0f - shoulder.y) + shoulder.y;
}
float dyeMixFactor(float mono, float maxDensity, const pt_tonemap_options& o) {
  float offset = exp2s(o.flim_sigmoid_log2_min);
  float fac = invLerp(log2s(mono + offset), o.flim_sigmoid_log2_min, o.flim_sigmoid_log2_max);
  fac = superSigmoid(fac, {o.flim_sigmoid_toe[0], o.flim_sigmoid_toe[1]}, {o.flim_sigmoid_shoulder[0], o.flim_sigmoid_shoulder[1]});
  fac *= maxDensity;
  fac = exp2s(-fac);
  return saturate(fac);
}
float3 colorLayer(float3 color, float3 sensitivityTone, float3 dyeTone, float maxDensity, const pt_tonemap_options& o) {
  sensitivityTone = sensitivityTone / rgbSum(sensitivityTone);
  dyeTone = dyeTone / rgbMax(dyeTone);
  float mono = dot(color, sensitivityTone);
  float mixFactor = dyeMixFactor(mono, maxDensity, o);
  return mix3(dyeTone, f3(1.0f), mixFactor);
}
float3 develop(float3 color, float exposure, float maxDensity, const pt_tonemap_options& o) {
  color *= exp2s(exposure);
  float3 result = colorLayer(color, f3(0, 0, 1), f3(1, 1, 0), maxDensity, o);
  result *= colorLayer(color, f3(0, 1, 0), f3(1, 0, 1), maxDensity, o);
  result *= colorLayer(color, f3(1, 0, 0), f3(0, 1, 1), maxDensity, o);
  return result;
}
float3 negativeAndPrint(float3 color, float3 backlight, const pt_tonemap_options& o) {
  color = develop(color, o.flim_negative_exposure, o.flim_negative_density, o);
  color *= backlight;
  return develop(color, o.flim_print_exposure, o.flim_print_density, o);
}
float3 apply(float3 val, const pt_tonemap_options& o) {
  val *= exp2s(o.flim_pre_exposure);
  Mat3 ext;
  ext.c0 = gamutRow(0.0f / 3.0f, o.flim_extended_gamut_scale[0], o.flim_extended_gamut_rotation[0], o.flim_extended_gamut_mul[0]);
  ext.c1 = gamutRow(1.0f / 3.0f, o.flim_extended_gamut_scale[1], o.flim_extended_gamut_rotation[1], o.flim_extended_gamut_mul[1]);
  ext.c2 = gamutRow(2.0f / 3.0f, o.flim_extended_gamut_scale[2], o.flim_extended_gamut_rotation[2], o.flim_extended_gamut_mul[2]);
  Mat3 extInv = inverse(ext);
  float3 backlight = vmul(f3(o.flim_print_backlight[0], o.flim_print_backlight[1], o.flim_print_backlight[2]), ext);
  float3 whiteCap = negativeAndPrint(f3(1e7f), backlight, o);
  float3 pre = f3(o.flim_pre_formation_filter[0], o.flim_pre_formation_filter[1], o.flim_pre_formation_filter[2]);
  val = mix3(val, val * pre, o.flim_pre_formation_filter_strength);
  val = vmul(val, ext);
  val = negativeAndPrint(val, backlight, o);
  val = vmul(val, extInv);
  val = f3(fmaxf(val.x, 0.0f), fmaxf(val.y, 0.0f), fmaxf(val.z, 0.0f));
  val = val / whiteCap;
  if (o.flim_auto_black_point) {
    float3 blackCap = negativeAndPrint(f3(0.0f), backlight, o);
    blackCap = blackCap / whiteCap;
    val = rgbUniformOffset(val, rgbAvg(blackCap) * 1000.0f, 0.0f);
  } else {
    val = rgbUniformOffset(val, o.flim_black_point, 0.0f);
  }
  float3 postf = f3(o.flim_post_formation_filter[0], o.flim_post_formation_filter[1], o.flim_post_formation_filter[2]);
  val = mix3(val, val * postf, o.flim_post_formation_filter_strength);
  val = sat3(val);
  float mono = rgbAvg(val);
  float mixFactor = (mono < 0.5f) ? invLerp(mono, 0.05f, 0.5f) : invLerp(mono, 0.95f, 0.5f);
  val = mix3(val, hueSat(val, 0.5f, o.flim_midtone_saturation, 1.0f), mixFactor);
  return sat3(val);
}
}  // namespace flim

inline float2 aspectCompensatedUv(float2 uv, float aspect) {  // :481-486
  if (aspect > 1.0f) uv.y = (uv.y - 0.5f) / aspect + 0.5f; else uv.x = (uv.x - 0.5f) * aspect + 0.5f;
  return uv;
}
inline float2 aspectCompensatedUvInverse(float2 uv, float aspect) {  // :488-493
  if (aspect > 1.0f) uv.y = (uv.y - 0.5f) * aspect + 0.5f; else uv.x = (uv.x - 0.5f) / aspect + 0.5f;
  return uv;
}

// src.sample(linear, clamp_to_edge) of the exposure pass' output, one channel (software bilinear, texel centres)
float sampleExposed(const float* acc, uint32_t W, uint32_t H, float expScale, float2 uv, int ch) {
  float fx = uv.x * (float)W - 0.5f, fy = uv.y * (float)H - 0.5f;
  float x0f = floorf(fx), y0f = floorf(fy);
  float wx = fx - x0f, wy = fy - y0f;
  int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  auto cl = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
  x0 = cl(x0, (int)W - 1); x1 = cl(x1, (int)W - 1); y0 = cl(y0, (int)H - 1); y1 = cl(y1, (int)H - 1);
  auto tap = [&](int x, int y) { return acc[4 * ((size_t)y * W + x) + ch] * expScale; };
  float t00 = tap(x0, y0), t01 = tap(x1, y0), t10 = tap(x0, y1), t11 = tap(x1, y1);
  float a = t00 + (t01 - t00) * wx, b = t10 + (t11 - t10) * wx;
  return a + (b - a) * wy;
}

inline float sRGB_channel(float c) { return c < 0.0031308f ? 12.92f * c : 1.055f * powrg(c, 1.0f / 2.4f) - 0.055f; }  // :29-32

// exposure -> chromaticAberration -> contrastSaturation -> toneCurve -> vignette -> tonemap for one pixel
float3 pixel(const float* acc, uint32_t W, uint32_t H, uint32_t px, uint32_t py, const pt_post_options& o, const pt_tonemap_options& t,
             const Mat3& odt) {
  float2 uv = {((float)px + 0.5f) / (float)W, ((float)py + 0.5f) / (float)H};
  float expScale = exp2s(o.exposure);
  const float* a = &acc[4 * ((size_t)py * W + px)];
  float3 color = f3(a[0], a[1], a[2]) * expScale;  // exposure, :425-437
  if (o.ca_amount != 0.0f) {  // chromaticAberration, :526-551
    float aspect = (float)W / (float)H;
    float2 uvM = aspectCompensatedUv(uv, aspect);
    float amount = o.ca_amount * 0.005f * 0.01f;
    float sr = 1.0f + amount, sg = 1.0f - amount * o.ca_green_shift * 0.01f, sb = 1.0f - amount;
    float2 uvR = aspectCompensatedUvInverse({(uvM.x - 0.5f) * sr + 0.5f, (uvM.y - 0.5f) * sr + 0.5f}, aspect);
    float2 uvG = aspectCompensatedUvInverse({(uvM.x - 0.5f) * sg + 0.5f, (uvM.y - 0.5f) * sg + 0.5f}, aspect);
    float2 uvB = aspectCompensatedUvInverse({(uvM.x - 0.5f) * sb + 0.5f, (uvM.y - 0.5f) * sb + 0.5f}, aspect);
    color.x = sampleExposed(acc, W, H, expScale, uvR, 0);
    color.y = sampleExposed(acc, W, H, expScale, uvG, 1);
    color.z = sampleExposed(acc, W, H, expScale, uvB, 2);
  }
  {  // contrastSaturation, :439-463
    const float eps = 1e-6f;
    float3 logColor = log2v(color + f3(eps));
    float3 adj = mix3(f3(0.18f), logColor, 1.0f + o.contrast * 0.01f);
    float3 e = exp2v(adj) - f3(eps);
    color = f3(fminf(fmaxf(e.x, 0.0f), ceiling), fminf(fmaxf(e.y, 0.0f), ceiling), fminf(fmaxf(e.z, 0.0f), ceiling));
    float3 gray = f3(luma(color));
    color = mix3(gray, color, 1.0f + o.saturation * 0.01f);
  }
  {  // toneCurve, :465-479
    float l = luma(color);
    float blacks = smoothstep(0.04f, 0.0f, l), shadows = smoothstep(0.18f, 0.0f, l);
    float highlights = smoothstep(0.18f, 1.0f, l), whites = smoothstep(0.75f, 1.0f, l);
    color *= exp2s(0.01f * o.blacks * blacks);
    color *= exp2s(0.01f * o.shadows * shadows);
    color *= exp2s(0.01f * o.highlights * highlights);
    color *= exp2s(0.01f * o.whites * whites);
  }
  {  // vignette, :495-524
    float aspect = (float)W / (float)H;
    aspect = mix(1.0f, aspect, o.vig_roundness * 0.01f);
    float2 uvM = aspectCompensatedUv(uv, aspect);
    float cornerToCenter = sqrtf(0.5f * 0.5f + 0.5f * 0.5f);
    float dx = uvM.x - 0.5f, dy = uvM.y - 0.5f;
    float distanceNorm = sqrtf(dx * dx + dy * dy) / cornerToCenter;
    float end = 1.0f - o.vig_midpoint * 0.01f;
    float start = end * (1.0f - o.vig_feather * 0.01f);
    float power = o.vig_power * 0.05f;
    float d = invLerp(distanceNorm, start, end);
    float vignetting = (d == 0.0f ? 0.0f : powrg(d, power)) * smoothstep(start, end, distanceNorm);
    color *= exp2s(o.vig_amount * vignetting);
  }
  switch (t.tonemapper) {  // tonemap, :553-600
    case 1: { float3 c = agx::apply(color, t); color = f3(powrg(c.x, 2.2f), powrg(c.y, 2.2f), powrg(c.z, 2.2f)); break; }
    case 2: color = khronos_apply(color, t); break;
    case 3: color = flim::apply(color, t); break;
    default: break;
  }
  float3 liftColor = f3(t.shadow_color[0], t.shadow_color[1], t.shadow_color[2]);
  liftColor = liftColor - f3(rgbAvg(liftColor));
  float3 gammaColor = f3(t.midtone_color[0], t.midtone_color[1], t.midtone_color[2]);
  gammaColor = gammaColor - f3(rgbAvg(gammaColor));
  float3 gainColor = f3(t.highlight_color[0], t.highlight_color[1], t.highlight_color[2]);
  gainColor = gainColor - f3(rgbAvg(gainColor));
  float3 lift = liftColor + f3(t.shadow_offset * 0.01f);
  float3 gain = (f3(1.0f) + gainColor) + f3(t.highlight_offset * 0.01f);
  float3 midGray = (f3(0.5f) + gammaColor) + f3(t.midtone_offset * 0.01f);
  float3 gamma = log2v((f3(0.5f) - lift) / (gain - lift)) / log2v(midGray);  // log10 ratio == log2 ratio
  float3 tt = sat3(f3(powrg(color.x, 1.0f / gamma.x), powrg(color.y, 1.0f / gamma.y), powrg(color.z, 1.0f / gamma.z)));
  color = lift + (gain - lift) * tt;
  color = mul(odt, color);
  return f3(sRGB_channel(color.x), sRGB_channel(color.y), sRGB_channel(color.z));
}

inline uint32_t pack_rgba8(float3 c) {  // RGBA8Unorm store: clamp, x255, round to nearest
  auto q = [](float v) -> uint32_t { if (!(v > 0.0f)) return 0u; if (v >= 1.0f) return 255u; return (uint32_t)(v * 255.0f + 0.5f); };
  return q(c.x) | (q(c.y) << 8) | (q(c.z) << 16) | (255u << 24);
}

}  // namespace post
