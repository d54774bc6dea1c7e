"""The record marshalling of the light probe's three sides (Renderer.debugLights, EmuScene.debugLights, OracleScene.debugLights) and the
bit comparison between them — TEST INFRASTRUCTURE.  The witness (light_witness.py) does not import this module."""
import ctypes as C

import numpy as np

from platinum_amd import abi


def probe(call, fn, records, roughness=1.0, metallic=0.0, transmission=0.0, dim=0, tables=abi.PT_LIGHT_TABLES_HBM, bounce=1, lastSpecular=False):
    """Renderer.debugLights' arguments and result through call(n, byref(args), in pointer, out pointer)"""
    rec = np.ascontiguousarray(records, dtype=np.float32)
    wi, wo = abi.PT_LIGHT_IN_WORDS[fn], abi.PT_LIGHT_OUT_WORDS[fn]
    assert rec.ndim == 2 and rec.shape[1] == (6 if fn == abi.PT_LIGHT_SAMPLE else 4)
    n = rec.shape[0]
    buf = np.zeros((n, wi), np.float32)
    buf[:, :rec.shape[1]] = rec
    out = np.full(n * wo, 0xdeadbeef, np.uint32)
    args = abi.LightProbeArgs(roughness, metallic, transmission, dim, tables, bounce, 1 if lastSpecular else 0)
    call(n, C.byref(args), buf.ctypes.data, out.ctypes.data)
    return out.view(abi.LIGHT_SAMPLE_DTYPE if fn == abi.PT_LIGHT_SAMPLE else abi.ENV_MISS_DTYPE)


def words(out):
    return np.ascontiguousarray(out).view(np.uint32).reshape(len(out), -1)


def same_bits(a, b, nan_payload=False):
    """Records a and b equal word for word.  nan_payload=True: two NaNs in the same float field count as equal whatever their sign and payload
    (0 / 0 is a NaN of either sign depending on the machine: x86 gives the negative one, gfx950 the positive one)."""
    wa, wb = words(a), words(b)
    eq = wa == wb
    if nan_payload:
        isnan = lambda w: (w & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
        floats = np.ones(wa.shape[1], bool)
        if wa.shape[1] == abi.PT_LIGHT_OUT_WORDS[abi.PT_LIGHT_SAMPLE]:
            floats[[0, 10, 11]] = False          # lit, dim, pad are integers
        else:
            floats[3] = False
        eq = eq | (isnan(wa) & isnan(wb) & floats[None, :])
    return bool(eq.all())


def first_difference(a, b):
    wa, wb = words(a), words(b)
    i = np.flatnonzero((wa != wb).any(1))
    return None if not i.size else (int(i[0]), a[i[0]], b[i[0]])
