"""jdamd.torchio.decode_jpeg on the GPU: the torchvision-shaped front end ([C, H, W] uint8 tensors
on the device, a list as one batch, ordered on torch's current stream).

References: jd_coef's plain reference / jdoracle.decode permuted to CHW, and the luma plane
(tests/format_cases.py).  Bar: bit-exact.
"""
import numpy as np
import pytest
import torch

import format_cases as fc
import jd_synth
import layout_cases as lc
from jdamd import torchio

pytestmark = pytest.mark.gpu


def _tensor(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8)


@pytest.fixture(scope="module")
def inputs():
    """Matrix cases of three layouts and one 641 x 481 4:2:0 image with DRI: (bytes, RGB ref
    [3, H, W], gray ref [1, H, W])."""
    out = []
    by_id = {c.id: c for c in lc.matrix_cases()}
    for cid in ("4:2:0-rst1", "4:4:4-rst0", "1x1,2x1,2x1-rst1"):
        c = by_id[cid]
        out.append((c.data, fc.permuted(c.ref, "chw"), fc.gray_of_case(c)[None]))
    data = jd_synth.encode(jd_synth.synth_pixels(641, 481, 31), 90, "4:2:0", 1)
    out.append((data, fc.stream_reference(data, "chw"), fc.stream_reference(data, "gray")[None]))
    return out


@pytest.mark.parametrize("mode", ["RGB", "GRAY"])
def test_single_and_list(inputs, mode):
    k = 1 if mode == "RGB" else 2
    one = torchio.decode_jpeg(_tensor(inputs[0][0]), device="cuda", mode=mode)
    assert isinstance(one, torch.Tensor) and one.dtype == torch.uint8 and one.device.type == "cuda"
    assert tuple(one.shape) == inputs[0][k].shape and one.is_contiguous()
    assert np.array_equal(one.cpu().numpy(), inputs[0][k])
    outs = torchio.decode_jpeg([_tensor(d) for d, _, _ in inputs], device="cuda:0", mode=mode)
    assert isinstance(outs, list) and len(outs) == len(inputs)
    for o, item in zip(outs, inputs):
        assert o.dtype == torch.uint8 and o.device == torch.device("cuda", 0)
        assert tuple(o.shape) == item[k].shape and o.shape[0] == (3 if mode == "RGB" else 1)
        assert np.array_equal(o.cpu().numpy(), item[k])


def test_on_a_side_stream(inputs):
    """Called inside torch.cuda.stream(s): the decode is ordered on s, and a consumer on s reads
    the pixels without another synchronise."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = torchio.decode_jpeg([_tensor(d) for d, _, _ in inputs], device="cuda")
        sums = [o.to(torch.int64).sum() for o in outs]  # enqueued on s behind the decode
        copies = [o.clone() for o in outs]
    s.synchronize()
    for c, t, item in zip(copies, sums, inputs):
        assert int(t.item()) == int(item[1].astype(np.int64).sum())
        assert np.array_equal(c.cpu().numpy(), item[1])


def test_bad_image_raises_naming_its_index(inputs):
    good = [_tensor(d) for d, _, _ in inputs[:3]]
    data = inputs[3][0]
    bad = _tensor(data[: len(data) // 2])
    with pytest.raises(RuntimeError, match=r"image 2\b"):
        torchio.decode_jpeg(good[:2] + [bad] + good[2:], device="cuda")
    # the cached decoder is still good afterwards
    o = torchio.decode_jpeg(good[0], device="cuda")
    assert np.array_equal(o.cpu().numpy(), inputs[0][1])
