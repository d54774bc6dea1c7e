"""ctypes wrapper of the emu_* functions of the host harness (tests/host_build.py: tests/_build/libptamd_host.so) — the host build of
the product's per-path stage functions (TEST HARNESS, see tests/emu/wavefront_emu.cpp).  bench.py's cpu_baseline renders through
EmuScene.render.  Never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from platinum_amd import abi  # noqa: E402

import host_build  # noqa: E402


def bind(L):
    """The argtypes of the emu_* functions on L, a library that holds the harness (host_build.load of it, or of a unit that includes it)."""
    L.emu_create.restype = C.c_void_p
    L.emu_create.argtypes = [C.POINTER(abi.SceneSnapshot), C.POINTER(abi.RenderParams), C.c_void_p, C.c_uint64]
    L.emu_destroy.argtypes = [C.c_void_p]
    L.emu_get_constants.argtypes = [C.c_void_p, C.POINTER(abi.Constants)]
    L.emu_get_lights.restype = C.c_uint32
    L.emu_get_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.emu_debug_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.emu_trace_primary.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.emu_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.emu_halton.restype = C.c_float
    L.emu_halton.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    return L


def bind_lights(L):
    """The functions of tests/emu/light_emu.cpp, which only the whole harness holds."""
    L.emu_light_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.LightProbeArgs), C.c_void_p, C.c_void_p]
    L.emu_get_env_alias.restype = C.c_uint64
    L.emu_get_env_alias.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.emu_shade_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]      # tests/emu/shade_emu.cpp
    return L


@functools.lru_cache(maxsize=None)
def lib():
    return bind_lights(bind(host_build.load()))


class EmuScene:
    def __init__(self, scene, params, L=None):
        self.L = lib() if L is None else L
        self.params = params
        self.snapshot = scene.snapshot()
        blob = open(abi.LUT_PATH, "rb").read()
        self._blob = C.create_string_buffer(blob, len(blob))
        self.h = self.L.emu_create(C.byref(self.snapshot.struct), C.byref(params), self._blob, len(blob))
        if not self.h:
            raise RuntimeError("emu_create failed")
        self.W, self.H = params.width, params.height

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def constants(self):
        c = abi.Constants()
        self.L.emu_get_constants(self.h, C.byref(c))
        return c

    def lights(self):
        arr = (abi.AreaLight * 65536)()
        n = self.L.emu_get_lights(self.h, arr, 65536)
        return list(arr)[:n]

    def envAlias(self):
        n = self.L.emu_get_env_alias(self.h, None, 0)
        arr = np.zeros(n, dtype=abi.ALIAS_DTYPE)
        if n:
            self.L.emu_get_env_alias(self.h, arr.ctypes.data, n)
        return arr

    def debugLights(self, fn, records, **args):
        """emu_light_probe, the host build of pt_light_probe.h: Renderer.debugLights' arguments and result (light_lib.probe)"""
        import light_lib

        def call(n, a, i, o):
            if self.L.emu_light_probe(self.h, fn, n, a, i, o) != 0:
                raise RuntimeError("emu_light_probe refused the call")
        return light_lib.probe(call, fn, records, **args)

    def debugShading(self, records):
        """emu_shade_probe, the host build of pt_shade_probe.h: Renderer.debugShading's argument and result"""
        rec = np.ascontiguousarray(records, dtype=abi.SHADE_PROBE_IN_DTYPE).reshape(-1)
        out = np.full(len(rec) * abi.PT_SHADE_PROBE_OUT_WORDS, 0xdeadbeef, np.uint32)
        if self.L.emu_shade_probe(self.h, len(rec), rec.ctypes.data, out.ctypes.data) != 0:
            raise RuntimeError("emu_shade_probe refused the call")
        return out.view(abi.SHADE_PROBE_OUT_DTYPE)

    def debug_sample(self, sample_idx):
        B = self.params.max_bounces
        rad = np.zeros((self.H, self.W, 4), dtype=np.float32)
        hits = np.zeros((B, self.H, self.W, 2), dtype=np.int32)
        self.L.emu_debug_sample(self.h, sample_idx, rad.ctypes.data, hits.ctypes.data)
        return rad, hits

    def trace_primary(self, sample_idx=0):
        out = np.zeros(self.W * self.H, dtype=[("t", "f4"), ("u", "f4"), ("v", "f4"), ("instance", "i4"), ("primitive", "i4")])
        self.L.emu_trace_primary(self.h, sample_idx, out.ctypes.data)
        return out.reshape(self.H, self.W)

    def render(self, first, ns, acc=None, acc_n0=0, threads=1):
        """Samples [first, first + ns) of every pixel folded into the running mean `acc` (acc_n0 samples already in it): the product's
        stage functions on `threads` host threads (bench.py's cpu_baseline, kind "same-kernels-host")."""
        if acc is None:
            acc = np.zeros((self.H, self.W, 4), dtype=np.float32)
        assert acc.dtype == np.float32 and acc.flags["C_CONTIGUOUS"] and acc.shape == (self.H, self.W, 4)
        self.L.emu_render(self.h, first, ns, acc.ctypes.data, acc_n0, threads)
        return acc

    def halton(self, i, d):
        return self.L.emu_halton(self.h, i, d)
