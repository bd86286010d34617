"""Output formats, the host side (no GPU): jd_output_bytes, the argument checks of
jdamd.Decoder and jdamd.torchio.decode_jpeg, and an audit of the gray reference the GPU tests
(tests/test_gpu_formats.py) compare against.
"""
import ctypes

import numpy as np
import pytest
import torch

import format_cases as fc
import jdamd
import layout_cases as lc

P, B, G = jdamd.JD_FLAG_OUT_PLANAR, jdamd.JD_FLAG_OUT_BGR, jdamd.JD_FLAG_OUT_GRAY
OTHER = (jdamd.JD_FLAG_TIMING | jdamd.JD_FLAG_FORCE_SYNC | jdamd.JD_FLAG_FORCE_LANES | jdamd.JD_FLAG_FANCY_UPSAMPLING |
         jdamd.JD_FLAG_FULL_PIECES | jdamd.JD_FLAG_ASYNC_DEPTH2 | jdamd.JD_FLAG_WORST_CASE_POOLS | (1 << 20))


def test_flag_values():
    assert (P, B, G) == (128, 256, 512)
    assert jdamd.JD_ABI_VERSION == 9 and jdamd.load_library().jd_abi_version() == 9


def test_output_bytes_valid_combinations(golden):
    seen = 0
    for e in golden:
        try:
            h = jdamd.parse(e["data"])
        except jdamd.JDError:
            continue
        seen += 1
        for flags in (0, P, B, P | B):
            assert jdamd.output_bytes(h, flags) == 3 * h.width * h.height
        assert jdamd.output_bytes(h, G) == h.width * h.height
    assert seen >= 5


def test_output_bytes_ignores_other_flags(golden):
    h = jdamd.parse(next(e["data"] for e in golden if e["file"].endswith("3_120x120.jpg")))
    for flags in (0, P, B, P | B, G):
        assert jdamd.output_bytes(h, flags | OTHER) == jdamd.output_bytes(h, flags)


def test_output_bytes_invalid(golden):
    lib = jdamd.load_library()
    h = jdamd._c_header(jdamd.parse(golden[0]["data"]))
    n = ctypes.c_size_t(12345)
    assert lib.jd_output_bytes(None, 0, ctypes.byref(n)) == jdamd.JD_ERR_INVALID_ARG
    assert lib.jd_output_bytes(ctypes.byref(h), 0, None) == jdamd.JD_ERR_INVALID_ARG
    for flags in (G | P, G | B, G | P | B):
        assert lib.jd_output_bytes(ctypes.byref(h), flags, ctypes.byref(n)) == jdamd.JD_ERR_INVALID_ARG
        with pytest.raises(jdamd.JDError):
            jdamd.output_bytes(jdamd.parse(golden[0]["data"]), flags)
    assert n.value == 12345  # untouched by the failed calls


def test_format_flags():
    assert jdamd.format_flags() == 0
    assert jdamd.format_flags("chw", "rgb") == P
    assert jdamd.format_flags("hwc", "bgr") == B
    assert jdamd.format_flags("chw", "bgr") == P | B
    assert jdamd.format_flags("hwc", "gray") == G and jdamd.format_flags("chw", "gray") == G


@pytest.mark.parametrize("kw", [dict(layout="nchw"), dict(layout="CHW"), dict(layout=None), dict(channels="rgba"),
                                dict(channels="GRAY"), dict(layout="chw", channels="yuv")])
def test_decoder_rejects_unknown_format(kw, monkeypatch):
    """ValueError before the library is touched: no jd_ctx_create (which would need a GPU), not
    even a load."""
    def no_load(*a, **k):
        raise AssertionError("library touched before the argument check")

    monkeypatch.setattr(jdamd, "load_library", no_load)
    with pytest.raises(ValueError):
        jdamd.Decoder(0, **kw)


def test_torchio_rejects_bad_input():
    from jdamd import torchio

    good = torch.zeros(16, dtype=torch.uint8)
    for bad in (torch.zeros(16, dtype=torch.int8), torch.zeros(16, dtype=torch.float32),
                torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((), dtype=torch.uint8), b"\xff\xd8", None):
        with pytest.raises(ValueError):
            torchio.decode_jpeg(bad)
        with pytest.raises(ValueError):
            torchio.decode_jpeg([good, bad])
    with pytest.raises(ValueError):
        torchio.decode_jpeg(good, mode="RGBA")
    with pytest.raises(ValueError):
        torchio.decode_jpeg([])
    with pytest.raises(ValueError):
        torchio.decode_jpeg(good, device="cpu")


def test_torchio_without_gpu_raises(golden, monkeypatch):
    """No GPU (here: none that torch reports, whatever the machine): a RuntimeError, no crash."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from jdamd import torchio

    data = next(e["data"] for e in golden if e["file"].endswith("3_120x120.jpg"))
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for arg in (t, [t, t]):
        with pytest.raises(RuntimeError):
            torchio.decode_jpeg(arg)


def test_gray_reference_audit():
    """The luma plane the gray GPU tests compare against: equal to every channel of the RGB
    reference on 1-component files, and different from every channel of it on at least 90 % of the
    colour cases (a kernel that stored R, G or B instead would fail there)."""
    cases = lc.matrix_cases() + lc.colour_cases() + lc.quant_cases()
    ngray = ncolour = distinct = 0
    for c in cases:
        g = fc.gray_of_case(c)
        assert g.shape == c.ref.shape[:2] and g.dtype == np.uint8
        if c.layout == "gray":
            ngray += 1
            for ch in range(3):
                assert np.array_equal(g, c.ref[..., ch]), c.id
        else:
            ncolour += 1
            distinct += all(not np.array_equal(g, c.ref[..., ch]) for ch in range(3))
    assert ngray >= 4 and ncolour >= 90
    assert distinct >= 0.9 * ncolour, (distinct, ncolour)


def test_gray_of_stream_agrees_with_coefficients():
    """The reference rebuilt from a stream (jdoracle.decode_coefs + idct + index arithmetic) equals
    the one from the coefficients, on one case of every layout (luma below the maximum factor
    included), so streams not built from coefficients have a trustworthy luma reference."""
    for c in lc.matrix_cases()[1::4]:
        assert np.array_equal(fc.gray_of_stream(c.data), fc.gray_of_case(c)), c.id


def test_align_cases_cover_every_width():
    cases = fc.align_cases()
    assert {(c.width, c.height) for c in cases} == {(w, h) for w in range(1, 25) for h in (1, 2, 17)}
    assert len(cases) == 3 * 72
