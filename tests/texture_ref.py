"""The texture filtering contract restated in double precision — TEST INFRASTRUCTURE shared by test_textures_env_alpha.py (the oracle's
tex_sample against it) and geometry_witness.py (the albedo of a textured first hit)."""
import numpy as np

f32 = np.float32


def _bilinear_repeat(px, u, v):
    """Independent double-precision restatement of the filtering contract (oracle/pt_oracle.cpp tex_sample)."""
    h, w, _ = px.shape
    x, y = float(f32(u)) * w - 0.5, float(f32(v)) * h - 0.5
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    wx, wy = x - x0, y - y0
    t = lambda xx, yy: px[yy % h, xx % w].astype(np.float64)
    a = t(x0, y0) * (1 - wx) + t(x0 + 1, y0) * wx
    b = t(x0, y0 + 1) * (1 - wx) + t(x0 + 1, y0 + 1) * wx
    return a * (1 - wy) + b * wy
