"""Host-side mirror of `pt::renderer_pt::Renderer` (src/renderer_pt/renderer_pt.hpp:28-73) over the C ABI.

Same method names and argument meaning as the reference class, so that parity tests read like calls into the
reference: startRender(...) / render() / status() / renderProgress() / renderTime() / selectKernel(...).
The float accumulator (never exported by the reference) is the parity surface.
"""
import ctypes as C

import numpy as np

from . import abi, scenes


def make_params(width, height, spp, max_bounces, flags=abi.FLAG_MULTISCATTER_GGX, integrator=abi.INTEGRATOR_MIS,
                working_space=scenes.BT2020, gmon_buckets=1, first_sample=0, samples_in_flight=0,
                external_accumulator=None, stream=None, nonfinite_policy=abi.NONFINITE_PROPAGATE, accel_structure=abi.ACCEL_AUTO):
    p = abi.RenderParams()
    p.accel_structure = accel_structure
    p.width, p.height, p.spp, p.gmon_buckets = width, height, spp, gmon_buckets
    p.flags, p.integrator = flags, integrator
    p.working_space = scenes.colorspace(working_space)
    p.max_bounces, p.first_sample, p.samples_in_flight = max_bounces, first_sample, samples_in_flight
    p.nonfinite_policy = nonfinite_policy
    p.external_accumulator = external_accumulator
    p.stream = stream
    return p


class Renderer:
    # renderer_pt.hpp:16-26
    Integrator_Simple, Integrator_MIS = abi.INTEGRATOR_SIMPLE, abi.INTEGRATOR_MIS
    Status_Blocked, Status_Ready, Status_Busy, Status_Done = 0, 1, 4, 8

    def __init__(self, device=0, lut_path=None, devices=None):
        """Renderer(device, queue, store) (renderer_pt.cpp:18-60). Raises if the HIP library or a GPU is missing.
        `devices` = a list of HIP device ordinals: a device group that shards every render's samples (include/ptamd.h)."""
        self._lib = abi.load_library()
        info = abi.CreateInfo()
        info.abi_version = abi.PT_ABI_VERSION
        info.device_ordinal = device
        if devices is not None:
            self._devices = (C.c_int32 * len(devices))(*devices)
            info.device_ordinals = self._devices
            info.device_count = len(devices)
        self._lut = open(lut_path or abi.LUT_PATH, "rb").read()
        self._lut_buf = C.create_string_buffer(self._lut, len(self._lut))
        info.lut_blob = C.addressof(self._lut_buf)
        info.lut_blob_size = len(self._lut)
        info.lut_path = None
        h = C.c_void_p()
        abi.check(self._lib, self._lib.pt_create(C.byref(info), C.byref(h)))
        self._h = h
        self._integrator = abi.INTEGRATOR_MIS  # renderer_pt.hpp:98
        self._params = None
        self.size = (0, 0)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # renderer_pt.hpp:47-53
    def selectedKernel(self):
        return self._integrator

    def selectKernel(self, k):
        self._integrator = k

    def startRender(self, scene, size, spp, gmonBuckets=1, workingSpace=scenes.BT2020, flags=abi.FLAG_MULTISCATTER_GGX,
                    max_bounces=50, first_sample=0, samples_in_flight=0, external_accumulator=None, stream=None,
                    nonfinite_policy=abi.NONFINITE_PROPAGATE, accel_structure=abi.ACCEL_AUTO):
        """startRender(camera, size, spp, gmonBuckets, workingSpace, flags) (renderer_pt.hpp:38-45).
        `scene` (a scenes.Scene holding the camera node) replaces the NodeID into Store."""
        p = make_params(int(size[0]), int(size[1]), spp, max_bounces, flags, self._integrator, workingSpace, gmonBuckets,
                        first_sample, samples_in_flight, external_accumulator, stream, nonfinite_policy, accel_structure)
        snap = scene.snapshot()
        abi.check(self._lib, self._lib.pt_start_render(self._h, C.byref(snap.struct), C.byref(p)))
        self._params = p
        self.size = (p.width, p.height)

    def render(self, max_spp=1):
        """render() (renderer_pt.cpp:113-197) encodes 1 spp per call; max_spp=0 enqueues all remaining."""
        abi.check(self._lib, self._lib.pt_render_step(self._h, max_spp))

    def wait(self):
        abi.check(self._lib, self._lib.pt_wait(self._h))

    def status(self):
        return self._lib.pt_status(self._h)

    def renderProgress(self):
        a, t = C.c_uint64(), C.c_uint64()
        abi.check(self._lib, self._lib.pt_progress(self._h, C.byref(a), C.byref(t)))
        return a.value, t.value

    def renderTime(self):
        return self._lib.pt_render_time_ms(self._h)

    def readbackAccumulator(self):
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_accumulator(self._h, out.ctypes.data))
        return out

    # renderer_pt.hpp:65-73: the option structs the UI edits every frame
    def postProcessOptions(self):
        o = abi.PostOptions()
        self._lib.pt_default_post_options(C.byref(o))
        return o

    def tonemapOptions(self):
        o = abi.TonemapOptions()
        self._lib.pt_default_tonemap_options(C.byref(o))
        return o

    def setPostProcessOptions(self, o):
        abi.check(self._lib, self._lib.pt_set_post_options(self._h, C.byref(o)))

    def setTonemapOptions(self, o):
        abi.check(self._lib, self._lib.pt_set_tonemap_options(self._h, C.byref(o)))

    def readbackRenderTarget(self):
        """readbackRenderTarget() (renderer_pt.cpp:1039-1059): (H, W, 4) uint8, post-processed + tonemapped."""
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.uint8)
        abi.check(self._lib, self._lib.pt_read_render_target(self._h, out.ctypes.data))
        return out

    def presentRenderTarget(self):
        """presentRenderTarget() (renderer_pt.hpp:55): (device address of the RGBA8 image, hipStream_t it is produced on)."""
        ptr, stream = C.c_void_p(), C.c_void_p()
        abi.check(self._lib, self._lib.pt_present_render_target(self._h, C.byref(ptr), C.byref(stream)))
        return ptr.value, stream.value

    # first-hit AOVs + denoiser (include/ptamd.h, ABI 5): no reference counterpart
    def denoiseOptions(self):
        """The options in effect (pt_default_denoise_options until setDenoiseOptions is called)."""
        if getattr(self, "_denoise", None) is None:
            self._denoise = abi.DenoiseOptions()
            self._lib.pt_default_denoise_options(C.byref(self._denoise))
        o = abi.DenoiseOptions()
        C.memmove(C.byref(o), C.byref(self._denoise), C.sizeof(o))
        return o

    def setDenoiseOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setDenoiseOptions(enabled=1).
        `enabled` takes effect at the next startRender, the filter fields at the next read or present."""
        o = self.denoiseOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_denoise_options(self._h, C.byref(o)))
        self._denoise = o

    def readbackAov(self, kind):
        """(H, W, 4) float32 running mean of AOV `kind` (abi.AOV_ALBEDO / AOV_NORMAL / AOV_MOMENTS)."""
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_aov(self._h, kind, out.ctypes.data))
        return out

    def readbackDenoised(self):
        """(H, W, 4) float32: the accumulator through the a-trous denoiser with the current options."""
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_denoised(self._h, out.ctypes.data))
        return out

    # firefly clamp ahead of the denoiser (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def despeckleOptions(self):
        """The options in effect (pt_default_despeckle_options until setDespeckleOptions is called)."""
        if getattr(self, "_despeckle", None) is None:
            self._despeckle = abi.DespeckleOptions()
            self._lib.pt_default_despeckle_options(C.byref(self._despeckle))
        o = abi.DespeckleOptions()
        C.memmove(C.byref(o), C.byref(self._despeckle), C.sizeof(o))
        return o

    def setDespeckleOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setDespeckleOptions(enabled=1, threshold=2.0).
        The options take effect at the next readbackDenoised, or read / present with apply_to_target."""
        o = self.despeckleOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_despeckle_options(self._h, C.byref(o)))
        self._despeckle = o

    # auto exposure (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def exposureOptions(self):
        """The options in effect (pt_default_exposure_options until setExposureOptions is called)."""
        if getattr(self, "_exposure", None) is None:
            self._exposure = abi.ExposureOptions()
            self._lib.pt_default_exposure_options(C.byref(self._exposure))
        o = abi.ExposureOptions()
        C.memmove(C.byref(o), C.byref(self._exposure), C.sizeof(o))
        return o

    def setExposureOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setExposureOptions(enabled=1, smoothing=0.5).
        The options take effect at the next readbackRenderTarget / presentRenderTarget; no restart is needed."""
        o = self.exposureOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_exposure_options(self._h, C.byref(o)))
        self._exposure = o

    def resetExposure(self):
        """Forgets the previously applied ev: the next metered target starts from its own target_ev."""
        abi.check(self._lib, self._lib.pt_reset_exposure(self._h))

    def readbackExposureMeter(self):
        """abi.ExposureMeter of the image a target read would show now; does not advance the smoothing state.  Blocks."""
        m = abi.ExposureMeter()
        abi.check(self._lib, self._lib.pt_read_exposure_meter(self._h, C.byref(m)))
        return m

    def debugExposure(self, rgba, rect=None, options=None, scaled=True):
        """The meter's three kernels on a host (H, W, 4) float32 image over rect = (x0, y0, x1, y1) (default: the whole image) with `options`
        (default: the current ones) and no smoothing state: (abi.ExposureMeter, the scaled image or None)."""
        img = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = img.shape[:2]
        o = self.exposureOptions() if options is None else options
        rc = None if rect is None else (C.c_uint32 * 4)(*rect)
        m = abi.ExposureMeter()
        out = np.empty((h, w, 4), np.float32) if scaled else None
        abi.check(self._lib, self._lib.pt_debug_exposure(self._h, img.ctypes.data, w, h, None if rc is None else C.addressof(rc), C.byref(o),
                                                         C.byref(m), None if out is None else out.ctypes.data))
        return m, out

    def debugMath(self, fn, a, b=None):
        """pt_debug_math: function abi.PT_MATH_* on the device, elementwise on the 4-byte arrays a (and b).  Returns (out0, out1) as uint32
        words (view them as float32 where the function returns floats); out1 is None for a function of one result and holds 2n words for
        PT_MATH_SAMPLE_COSINE_HEMISPHERE (y, then z)."""
        a = np.ascontiguousarray(a)
        b = None if b is None else np.ascontiguousarray(b)
        assert a.dtype.itemsize == 4 and a.ndim == 1 and (b is None or (b.dtype.itemsize == 4 and b.shape == a.shape))
        n = a.size
        two = fn in (abi.PT_MATH_SINCOS, abi.PT_MATH_SAMPLE_DISK, abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE, abi.PT_MATH_SAMPLE_TRI_UNIFORM)
        out0 = np.empty(n, np.uint32)
        out1 = np.empty(2 * n if fn == abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE else n, np.uint32) if two else None
        abi.check(self._lib, self._lib.pt_debug_math(self._h, fn, n, a.ctypes.data, None if b is None else b.ctypes.data, out0.ctypes.data,
                                                     None if out1 is None else out1.ctypes.data))
        return out0, out1

    def debugLights(self, fn, records, roughness=1.0, metallic=0.0, transmission=0.0, dim=0, tables=abi.PT_LIGHT_TABLES_HBM, bounce=1,
                    lastSpecular=False):
        """pt_debug_lights on the scene of the started render.  fn = abi.PT_LIGHT_SAMPLE: `records` is (n, 6) float32, a hit position and the
        three NEE draws (rl.x, rl.y, rz); returns n records of abi.LIGHT_SAMPLE_DTYPE, shade_nee_light for a material with the given roughness /
        metallic / transmission at sampler cursor `dim`, its light table in HBM or staged in LDS (`tables`).  fn = abi.PT_LIGHT_ENV_MISS:
        `records` is (n, 4), a direction and lastPdf; returns n records of abi.ENV_MISS_DTYPE, stage_miss with attenuation 1 at `bounce`."""
        rec = np.ascontiguousarray(records, dtype=np.float32)
        wi, wo = abi.PT_LIGHT_IN_WORDS[fn], abi.PT_LIGHT_OUT_WORDS[fn]
        assert rec.ndim == 2 and rec.shape[1] == (6 if fn == abi.PT_LIGHT_SAMPLE else 4)
        n = rec.shape[0]
        buf = np.zeros((n, wi), np.float32)
        buf[:, :rec.shape[1]] = rec
        out = np.empty(n * wo, np.uint32)
        args = abi.LightProbeArgs(roughness, metallic, transmission, dim, tables, bounce, 1 if lastSpecular else 0)
        abi.check(self._lib, self._lib.pt_debug_lights(self._h, fn, n, C.byref(args), buf.ctypes.data, out.ctypes.data))
        return out.view(abi.LIGHT_SAMPLE_DTYPE if fn == abi.PT_LIGHT_SAMPLE else abi.ENV_MISS_DTYPE)

    def debugShading(self, records):
        """pt_debug_shading on the scene of the started render.  `records` is an array of abi.SHADE_PROBE_IN_DTYPE: a hit (instance, primitive,
        u, v) and its ray (o, d, t); returns as many records of abi.SHADE_PROBE_OUT_DTYPE: hitPos, the shading frame, wo and the shading context
        as the shade and AOV kernels compute them for that hit, and the triangle's material class."""
        rec = np.ascontiguousarray(records, dtype=abi.SHADE_PROBE_IN_DTYPE).reshape(-1)
        out = np.empty(len(rec) * abi.PT_SHADE_PROBE_OUT_WORDS, np.uint32)
        abi.check(self._lib, self._lib.pt_debug_shading(self._h, len(rec), rec.ctypes.data, out.ctypes.data))
        return out.view(abi.SHADE_PROBE_OUT_DTYPE)

    # bloom (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def bloomOptions(self):
        """The options in effect (pt_default_bloom_options until setBloomOptions is called)."""
        if getattr(self, "_bloom", None) is None:
            self._bloom = abi.BloomOptions()
            self._lib.pt_default_bloom_options(C.byref(self._bloom))
        o = abi.BloomOptions()
        C.memmove(C.byref(o), C.byref(self._bloom), C.sizeof(o))
        return o

    def setBloomOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setBloomOptions(enabled=1, intensity=0.1).
        The options take effect at the next readbackRenderTarget / presentRenderTarget; no restart is needed."""
        o = self.bloomOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_bloom_options(self._h, C.byref(o)))
        self._bloom = o

    def debugBloom(self, rgba, options=None, pyramid=False):
        """Bloom's launches on a host (H, W, 4) float32 image with `options` (default: the current ones; `enabled` is not looked at): the
        bloomed image, or with pyramid=True (image, U_1..U_L as an (abi.BloomPlan.total_texels, 4) array laid out by pt_plan_bloom)."""
        img = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = img.shape[:2]
        o = self.bloomOptions() if options is None else options
        out = np.empty((h, w, 4), np.float32)
        pyr = None
        if pyramid:
            plan = abi.BloomPlan()
            abi.check(self._lib, self._lib.pt_plan_bloom(w, h, o.levels, C.byref(plan)))
            pyr = np.zeros((plan.total_texels, 4), np.float32)
        abi.check(self._lib, self._lib.pt_debug_bloom(self._h, img.ctypes.data, w, h, C.byref(o), out.ctypes.data,
                                                      None if pyr is None or pyr.size == 0 else pyr.ctypes.data))
        return (out, pyr) if pyramid else out

    # sun and sky (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def skyOptions(self, **fields):
        """pt_default_sky_options with `fields` over them, e.g. skyOptions(sun_elevation=0.1, dust_density=3)."""
        o = abi.SkyOptions()
        self._lib.pt_default_sky_options(C.byref(o))
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    def generateSky(self, options=None, width=1024, height=512, stats=False, **fields):
        """pt_generate_sky: the (height, width, 4) float32 lat-long image of the single-scattering sky under `options` (default: skyOptions
        of `fields`), in the environment map's layout; with stats=True (image, abi.SkyStats).  Needs no started render."""
        o = self.skyOptions(**fields) if options is None else options
        out = np.empty((height, width, 4), np.float32)
        st = abi.SkyStats()
        abi.check(self._lib, self._lib.pt_generate_sky(self._h, C.byref(o), width, height, out.ctypes.data, C.byref(st)))
        return (out, st) if stats else out

    # tile-adaptive sampling (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def adaptiveOptions(self):
        """The options in effect (pt_default_adaptive_options until setAdaptiveOptions is called)."""
        if getattr(self, "_adaptive", None) is None:
            self._adaptive = abi.AdaptiveOptions()
            self._lib.pt_default_adaptive_options(C.byref(self._adaptive))
        o = abi.AdaptiveOptions()
        C.memmove(C.byref(o), C.byref(self._adaptive), C.sizeof(o))
        return o

    def setAdaptiveOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setAdaptiveOptions(enabled=1, threshold=0.05).
        The options take effect at the next startRender."""
        o = self.adaptiveOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_adaptive_options(self._h, C.byref(o)))
        self._adaptive = o

    def readbackSampleCounts(self):
        """(H, W) uint32: the samples folded into each pixel (its 8x8 tile's count; uniform for a non-adaptive render)."""
        w, h = self.size
        out = np.empty((h, w), dtype=np.uint32)
        abi.check(self._lib, self._lib.pt_read_sample_counts(self._h, out.ctypes.data))
        return out

    # render regions (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def renderRegion(self):
        """The region in effect (pt_default_render_region, the whole frame, until setRenderRegion is called)."""
        if getattr(self, "_region", None) is None:
            self._region = abi.RenderRegion()
            self._lib.pt_default_render_region(C.byref(self._region))
        o = abi.RenderRegion()
        C.memmove(C.byref(o), C.byref(self._region), C.sizeof(o))
        return o

    def setRenderRegion(self, x0, y0, x1, y1):
        """The next startRender samples only the pixels [x0, x1) x [y0, y1) (top-left origin)."""
        o = abi.RenderRegion(1, x0, y0, x1, y1)
        abi.check(self._lib, self._lib.pt_set_render_region(self._h, C.byref(o)))
        self._region = o

    def clearRenderRegion(self):
        """The next startRender samples the whole frame again."""
        o = abi.RenderRegion()
        self._lib.pt_default_render_region(C.byref(o))
        abi.check(self._lib, self._lib.pt_set_render_region(self._h, C.byref(o)))
        self._region = o

    # ID mattes (include/ptamd.h, an additive extension of ABI 5): no reference counterpart
    def matteOptions(self):
        """The options in effect (pt_default_matte_options until setMatteOptions is called)."""
        if getattr(self, "_matte", None) is None:
            self._matte = abi.MatteOptions()
            self._lib.pt_default_matte_options(C.byref(self._matte))
        o = abi.MatteOptions()
        C.memmove(C.byref(o), C.byref(self._matte), C.sizeof(o))
        return o

    def setMatteOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setMatteOptions(enabled=1).
        The options take effect at the next startRender."""
        o = self.matteOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_matte_options(self._h, C.byref(o)))
        self._matte = o

    def readbackMatteSlots(self, layer):
        """(H, W, abi.MATTE_SLOTS) records {id, count} of layer abi.MATTE_INSTANCE / MATTE_MATERIAL, each pixel's slots in first-seen order;
        an empty slot is {abi.MATTE_NONE, 0}."""
        w, h = self.size
        out = np.empty((h, w, abi.MATTE_SLOTS), dtype=abi.MATTE_SLOT_DTYPE)
        abi.check(self._lib, self._lib.pt_read_matte_slots(self._h, layer, out.ctypes.data))
        return out

    def readbackMatte(self, layer, ids):
        """(H, W) float32 coverage of the ids (any iterable of instance or material indices; abi.MATTE_NONE selects the background)."""
        w, h = self.size
        ids = np.ascontiguousarray(np.asarray(list(ids), dtype=np.uint32).reshape(-1))
        out = np.empty((h, w), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_matte(self._h, layer, ids.ctypes.data if ids.size else None, ids.size, out.ctypes.data))
        return out

    def pick(self, x, y):
        """abi.PickResult of pixel (x, y), top-left origin: what most of its camera samples hit first."""
        out = abi.PickResult()
        abi.check(self._lib, self._lib.pt_pick(self._h, x, y, C.byref(out)))
        return out

    # selection overlay (include/ptamd.h, an additive extension of ABI 5): no counterpart in the reference's path tracer
    def selectionOptions(self):
        """The options in effect (pt_default_selection_options until setSelectionOptions is called)."""
        if getattr(self, "_selection", None) is None:
            self._selection = abi.SelectionOptions()
            self._lib.pt_default_selection_options(C.byref(self._selection))
        o = abi.SelectionOptions()
        C.memmove(C.byref(o), C.byref(self._selection), C.sizeof(o))
        return o

    def setSelectionOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setSelectionOptions(enabled=1, width=3.0,
        outline_rgba=(0, 1, 1, 1)).  The options take effect at the next readbackRenderTarget / presentRenderTarget; no restart is needed."""
        o = self.selectionOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, (C.c_float * 4)(*v) if k in ("outline_rgba", "fill_rgba") else v)
        abi.check(self._lib, self._lib.pt_set_selection_options(self._h, C.byref(o)))
        self._selection = o

    def setSelection(self, ids):
        """The selected ids of selectionOptions().layer (any iterable; abi.MATTE_NONE selects the background; empty clears the selection)."""
        ids = np.ascontiguousarray(np.asarray(list(ids), dtype=np.uint32).reshape(-1))
        abi.check(self._lib, self._lib.pt_set_selection(self._h, ids.ctypes.data if ids.size else None, ids.size))

    def selection(self):
        """The stored selection: uint32 ids, ascending, without duplicates."""
        n = C.c_uint32()
        abi.check(self._lib, self._lib.pt_get_selection(self._h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        abi.check(self._lib, self._lib.pt_get_selection(self._h, out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out

    def debugSelectionOverlay(self, rgba8, coverage, options=None):
        """The overlay kernel on a host (H, W, 4) uint8 target and an (H, W) float32 coverage image with `options` (default: the current
        ones; `enabled` is not looked at): the target with the outline and the tint drawn."""
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        h, w = img.shape[:2]
        cov = np.ascontiguousarray(coverage, dtype=np.float32)
        assert img.shape == (h, w, 4) and cov.shape == (h, w)
        o = self.selectionOptions() if options is None else options
        out = np.empty((h, w, 4), np.uint8)
        abi.check(self._lib, self._lib.pt_debug_selection_overlay(self._h, img.ctypes.data, cov.ctypes.data, w, h, C.byref(o), out.ctypes.data))
        return out

    # transparent film (include/ptamd.h, an additive extension of ABI 5): no counterpart in the reference's path tracer
    def filmOptions(self):
        """The options in effect (pt_default_film_options until setFilmOptions is called)."""
        if getattr(self, "_film", None) is None:
            self._film = abi.FilmOptions()
            self._lib.pt_default_film_options(C.byref(self._film))
        o = abi.FilmOptions()
        C.memmove(C.byref(o), C.byref(self._film), C.sizeof(o))
        return o

    def setFilmOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setFilmOptions(enabled=1,
        backdrop=abi.BACKDROP_COLOR, backdrop_rgb=(0.2, 0.2, 0.2)).  `enabled` takes effect at the next startRender; the backdrop at the
        next readbackRenderTarget / presentRenderTarget, without a restart."""
        o = self.filmOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, (C.c_float * 3)(*v) if k == "backdrop_rgb" else v)
        abi.check(self._lib, self._lib.pt_set_film_options(self._h, C.byref(o)))
        self._film = o

    def readbackFilm(self):
        """(H, W, 4) float32 {premultiplied foreground rgb, coverage} of a render started with the film enabled."""
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_film(self._h, out.ctypes.data))
        return out

    # camera projections (include/ptamd.h, an additive extension of ABI 5): no counterpart in the reference's path tracer
    def projection(self):
        """The projection the NEXT startRender will use (pt_default_camera_projection until setProjection is called)."""
        if getattr(self, "_projection", None) is None:
            self._projection = abi.CameraProjection()
            self._lib.pt_default_camera_projection(C.byref(self._projection))
        o = abi.CameraProjection()
        C.memmove(C.byref(o), C.byref(self._projection), C.sizeof(o))
        return o

    def setProjection(self, o=None, **fields):
        """Sets `o` (default: the current projection) with `fields` overriding it, e.g. setProjection(kind=abi.PROJ_EQUIRECT) or
        setProjection(kind=abi.PROJ_ORTHOGRAPHIC, ortho_height=2.5).  Takes effect at the next startRender."""
        o = self.projection() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_camera_projection(self._h, C.byref(o)))
        self._projection = o

    def renderProjection(self):
        """The projection the current render was started with."""
        o = abi.CameraProjection()
        abi.check(self._lib, self._lib.pt_get_camera_projection(self._h, C.byref(o)))
        return o

    def debugCameraRays(self, sample_idx=0):
        """(origins, directions), each (H, W, 3) float32: the camera rays of one sample as the render's own ray-generation kernel makes them."""
        w, h = self.size
        o, d = np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32)
        abi.check(self._lib, self._lib.pt_debug_camera_rays(self._h, sample_idx, o.ctypes.data, d.ctypes.data))
        return o, d

    # ambient occlusion (include/ptamd.h, an additive extension of ABI 5): no counterpart in the reference's path tracer
    def ambientOcclusionOptions(self):
        """The options in effect (pt_default_ao_options until setAmbientOcclusionOptions is called)."""
        if getattr(self, "_ao", None) is None:
            self._ao = abi.AoOptions()
            self._lib.pt_default_ao_options(C.byref(self._ao))
        o = abi.AoOptions()
        C.memmove(C.byref(o), C.byref(self._ao), C.sizeof(o))
        return o

    def setAmbientOcclusionOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setAmbientOcclusionOptions(enabled=1, distance=2.0);
        distance may be float("inf").  Takes effect at the next startRender."""
        o = self.ambientOcclusionOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_ao_options(self._h, C.byref(o)))
        self._ao = o

    def readbackAmbientOcclusion(self):
        """(H, W) float32: open / hits per pixel (1 where no camera ray hit) of a render started with ambient occlusion enabled."""
        w, h = self.size
        out = np.empty((h, w), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_ao(self._h, out.ctypes.data))
        return out

    def readbackAmbientOcclusionCounts(self):
        """(H, W, 2) uint32 {hits, open}: the camera rays of the pixel's samples that hit, and those of them whose AO ray met nothing."""
        w, h = self.size
        out = np.empty((h, w, 2), dtype=np.uint32)
        abi.check(self._lib, self._lib.pt_read_ao_counts(self._h, out.ctypes.data))
        return out

    def debugAmbientOcclusion(self, sample_idx=0):
        """(origins, directions, state): (H, W, 3) float32 twice and (H, W) uint32 (abi.AO_MISS / AO_OCCLUDED / AO_OPEN): the AO rays of one
        sample of every pixel as the render's own trace kernel makes them; zero origin and direction where the camera ray missed."""
        w, h = self.size
        o, d, st = np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32), np.empty((h, w), np.uint32)
        abi.check(self._lib, self._lib.pt_debug_ao(self._h, sample_idx, o.ctypes.data, d.ctypes.data, st.ctypes.data))
        return o, d, st

    def ambientOcclusionStats(self):
        s = abi.AoStats()
        abi.check(self._lib, self._lib.pt_get_ao_stats(self._h, C.byref(s)))
        return s

    # pass views (include/ptamd.h, an additive extension of ABI 5): no counterpart in the reference's path tracer
    def viewOptions(self):
        """The options in effect (pt_default_view_options until setViewOptions is called)."""
        if getattr(self, "_view", None) is None:
            self._view = abi.ViewOptions()
            self._lib.pt_default_view_options(C.byref(self._view))
        o = abi.ViewOptions()
        C.memmove(C.byref(o), C.byref(self._view), C.sizeof(o))
        return o

    def setViewOptions(self, o=None, **fields):
        """Sets `o` (default: the current options) with `fields` overriding it, e.g. setViewOptions(view=abi.VIEW_DEPTH,
        ramp=abi.RAMP_HEAT).  The view takes effect at the next readbackRenderTarget / presentRenderTarget; no restart is needed."""
        o = self.viewOptions() if o is None else o
        for k, v in fields.items():
            setattr(o, k, v)
        abi.check(self._lib, self._lib.pt_set_view_options(self._h, C.byref(o)))
        self._view = o

    def viewStats(self):
        """abi.ViewStats: the view the target shows now (VIEW_BEAUTY when the one asked for is not available) and, under VIEW_DEPTH, the
        range in use.  Blocks; draws nothing."""
        s = abi.ViewStats()
        abi.check(self._lib, self._lib.pt_read_view_stats(self._h, C.byref(s)))
        return s

    def debugView(self, size, options=None, rect=None, spp=1, counts=None, normal=None, moments=None, film=None, slots=None):
        """The data-view kernels on host images of `size` = (W, H) with `options` (default: the current ones): ((H, W, 4) uint8,
        abi.ViewStats).  counts (H, W) uint32; normal / moments / film (H, W, 4) float32; slots (H, W, MATTE_SLOTS) of one layer."""
        w, h = size
        keep = []

        def ptr(a, dtype, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            assert a.shape == shape, (a.shape, shape)
            keep.append(a)
            return a.ctypes.data

        inp = abi.ViewInputs(None, ptr(normal, np.float32, (h, w, 4)), ptr(moments, np.float32, (h, w, 4)), ptr(film, np.float32, (h, w, 4)),
                             ptr(slots, np.dtype(abi.MATTE_SLOT_DTYPE), (h, w, abi.MATTE_SLOTS)), ptr(counts, np.uint32, (h, w)), spp)
        o = self.viewOptions() if options is None else options
        r = None if rect is None else (C.c_uint32 * 4)(*rect)
        out = np.empty((h, w, 4), np.uint8)
        stats = abi.ViewStats()
        abi.check(self._lib, self._lib.pt_debug_view(self._h, C.byref(inp), w, h, r, C.byref(o), out.ctypes.data, C.byref(stats)))
        return out, stats

    def setGmonOptions(self, cap=1.0):
        """gmonOptions().cap (renderer_pt.hpp:71)."""
        o = abi.GmonOptions(cap)
        abi.check(self._lib, self._lib.pt_set_gmon_options(self._h, C.byref(o)))

    def readGmonBucket(self, bucket):
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        abi.check(self._lib, self._lib.pt_read_gmon_bucket(self._h, bucket, out.ctypes.data))
        return out

    def accumulatorDevicePtr(self):
        return self._lib.pt_accumulator_device_ptr(self._h)

    # ---- parity / measurement surface ----
    def constants(self):
        c = abi.Constants()
        abi.check(self._lib, self._lib.pt_get_constants(self._h, C.byref(c)))
        return c

    def lights(self):
        n = C.c_uint32()
        abi.check(self._lib, self._lib.pt_get_lights(self._h, None, 0, C.byref(n)))
        arr = (abi.AreaLight * max(1, n.value))()
        abi.check(self._lib, self._lib.pt_get_lights(self._h, arr, n.value, C.byref(n)))
        return list(arr)[: n.value]

    def envAlias(self):
        """The environment alias table in use (Environment::rebuildAliasTable, core/environment.cpp:5-91)."""
        n = C.c_uint64()
        abi.check(self._lib, self._lib.pt_get_env_alias(self._h, None, 0, C.byref(n)))
        arr = np.zeros(n.value, dtype=abi.ALIAS_DTYPE)
        if n.value:
            abi.check(self._lib, self._lib.pt_get_env_alias(self._h, arr.ctypes.data, n.value, C.byref(n)))
        return arr

    def tracePrimary(self, sample_idx=0):
        w, h = self.size
        out = np.zeros(w * h, dtype=[("t", "f4"), ("u", "f4"), ("v", "f4"), ("instance", "i4"), ("primitive", "i4")])
        abi.check(self._lib, self._lib.pt_trace_primary(self._h, sample_idx, out.ctypes.data))
        return out.reshape(h, w)

    def debugSample(self, sample_idx):
        w, h = self.size
        B = self._params.max_bounces
        rad = np.zeros((h, w, 4), dtype=np.float32)
        hits = np.zeros((B, h, w, 2), dtype=np.int32)
        abi.check(self._lib, self._lib.pt_debug_sample(self._h, sample_idx, rad.ctypes.data, hits.ctypes.data))
        return rad, hits

    def stats(self):
        s = abi.Stats()
        abi.check(self._lib, self._lib.pt_get_stats(self._h, C.byref(s)))
        return s

    def cameraListStats(self):
        """pt_get_camera_list_stats: the per-pixel leaf lists the camera rays of this render are traced from (built = 0: none)."""
        s = abi.CameraListStats()
        abi.check(self._lib, self._lib.pt_get_camera_list_stats(self._h, C.byref(s)))
        return s

    def setProfiling(self, enabled):
        abi.check(self._lib, self._lib.pt_set_profiling(self._h, int(enabled)))

    def measureTraversal(self, sample_idx=0):
        abi.check(self._lib, self._lib.pt_measure_traversal(self._h, sample_idx))
