"""References for the output formats (JD_FLAG_OUT_PLANAR / _BGR / _GRAY), shared by
tests/test_formats_abi.py (CPU), tests/test_gpu_formats.py and tests/test_gpu_torchio.py (GPU).

Nothing here depends on a decoder's output: planar and BGR references are numpy permutations of an
interleaved RGB reference (jd_coef's plain reference or jdoracle.decode); the gray reference is the
luma plane, clip(Y + 128, 0, 255), either from the coefficients a case was built from (c.ycc[0]) or,
for any stream, rebuilt from jdoracle.decode_coefs: dequantised, through jdoracle.idct, replicated by
index arithmetic [y * v0 / vmax, x * h0 / hmax] and cropped.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "gpu-jpeg-decoder_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import jd_coef  # noqa: E402
import jdoracle  # noqa: E402

# name -> Decoder(layout=, channels=)
FORMATS = {"chw": ("chw", "rgb"), "bgr": ("hwc", "bgr"), "chw-bgr": ("chw", "bgr"), "gray": ("hwc", "gray")}
COLOUR_FORMATS = ["chw", "bgr", "chw-bgr"]


def permuted(rgb, fmt):
    """Interleaved RGB [H, W, 3] -> what format `fmt` (not gray) holds."""
    layout, channels = FORMATS[fmt]
    a = rgb[..., ::-1] if channels == "bgr" else rgb
    return np.ascontiguousarray(a.transpose(2, 0, 1) if layout == "chw" else a)


def gray_of_case(c):
    """The luma reference of a layout_cases case (built from its coefficients)."""
    return np.clip(c.ycc[0] + 128, 0, 255).astype(np.uint8)


def case_reference(c, fmt):
    return gray_of_case(c) if fmt == "gray" else permuted(c.ref, fmt)


def _tables(data):
    """(quant tables {id: int64[64], zig-zag order}, SOF0 components [(id, h, v, tq)], width, height)."""
    q, comps, w, h = {}, [], 0, 0
    i = 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF, "marker expected"
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        if m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                k += 1
                if pq:
                    q[tq] = np.array([(seg[k + 2 * j] << 8) | seg[k + 2 * j + 1] for j in range(64)], np.int64)
                    k += 128
                else:
                    q[tq] = np.array(list(seg[k:k + 64]), np.int64)
                    k += 64
        elif m == 0xC0:
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDA:
            break
        i += 2 + n
    return q, comps, w, h


def gray_of_stream(data):
    """The luma reference of any baseline stream: clip(Y + 128, 0, 255), uint8 [H, W]."""
    q, comps, w, h = _tables(data)
    st, coefs = jdoracle.decode_coefs(data)
    assert st == 0
    eff = [(1, 1)] if len(comps) == 1 else [(ch, cv) for _, ch, cv, _ in comps]
    hmax, vmax = max(a for a, _ in eff), max(b for _, b in eff)
    bpm = sum(a * b for a, b in eff)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    h0, v0 = eff[0]
    blocks = coefs.reshape(mcuy, mcux, bpm, 64)[:, :, :h0 * v0].astype(np.int64) * q[comps[0][3]]
    px = jdoracle.idct(blocks.reshape(-1, 64)).reshape(mcuy, mcux, v0, h0, 8, 8)
    plane = px.transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * v0 * 8, mcux * h0 * 8)
    ys = np.arange(h) * v0 // vmax
    xs = np.arange(w) * h0 // hmax
    return np.clip(plane[np.ix_(ys, xs)] + 128, 0, 255).astype(np.uint8)


def stream_reference(data, fmt, fancy=False):
    if fmt == "gray":
        return gray_of_stream(data)
    st, ref = jdoracle.decode(data, fancy=fancy)
    assert st == 0
    return permuted(ref, fmt)


# Store alignment and bounds: every width 1 .. 24 at heights 1, 2 and 17, random coefficients, built
# as layout_cases builds its cases.
ALIGN_LAYOUTS = {"gray": [(1, 1)], "4:4:4": [(1, 1), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)]}


@functools.lru_cache(None)
def align_cases():
    import layout_cases as lc
    from types import SimpleNamespace

    out = []
    rng = np.random.default_rng(777)
    for name, f in ALIGN_LAYOUTS.items():
        for height in (1, 2, 17):
            for width in range(1, 25):
                coefs = []
                for s in jd_coef.coef_shapes(width, height, f):
                    a = rng.integers(-60, 61, s) * (rng.random(s) < 0.3)
                    a[..., 0] = rng.integers(-900, 901, s[:-1])
                    coefs.append(a.astype(np.int32))
                qt = [lc.Q_LUMA, lc.Q_CHROMA]
                data = jd_coef.build(width, height, f, coefs, qt)
                ycc = jd_coef.upsampled(width, height, f, jd_coef.planes(width, height, f, coefs, qt))
                out.append(SimpleNamespace(id=f"{name}-{width}x{height}", width=width, height=height, data=data, ycc=ycc,
                                           ref=jd_coef.colour(*ycc)))
    return out
