"""jdamd.torchio — a torch front end: decode_jpeg(), a drop-in for
torchvision.io.decode_jpeg(input, device="cuda", mode=...) on ROCm.

    from jdamd.torchio import decode_jpeg
    imgs = decode_jpeg([torch.frombuffer(b, dtype=torch.uint8) for b in files], device="cuda")

The outputs are uint8 [3, H, W] (mode="RGB") or [1, H, W] (mode="GRAY") tensors on the device,
written by the decoder's colour stage in that layout (JD_FLAG_OUT_PLANAR / JD_FLAG_OUT_GRAY): no
permute, no second pass over the pixels.  A list is one jd_decode_batch call, ordered on torch's
current stream of the device.

torch is imported before libjdamd.so is loaded: PyTorch-ROCm bundles its own HIP runtime under the
soname the library links, and whichever loads first serves the process (a torch that finds the
system runtime already loaded reports no GPUs).

Threading: one Decoder is cached per (device index, mode) and closed at interpreter exit.  A
jd_ctx belongs to one host thread (include/jd.h), so a cached decoder belongs to the thread that
first used it: call decode_jpeg for one device from one thread, or create Decoders of your own.
"""
from __future__ import annotations

import atexit
import ctypes
from typing import Dict, List, Sequence, Tuple, Union

import torch  # before load_library(), see above

import jdamd

MODES = {"RGB": ("chw", "rgb"), "GRAY": ("chw", "gray")}
_decoders: Dict[Tuple[int, str], "jdamd.Decoder"] = {}


def _close_all() -> None:
    for dec in _decoders.values():
        try:
            dec.close()
        except Exception:
            pass
    _decoders.clear()


atexit.register(_close_all)


def _check_input(t, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expected a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: expected a uint8 tensor, not {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{what}: expected a 1-D tensor, not {t.dim()}-D")
    if t.device.type != "cpu":
        raise ValueError(f"{what}: expected a CPU tensor (the encoded bytes), not one on {t.device}")
    if t.numel() == 0:
        raise ValueError(f"{what}: empty tensor")


def _decoder(index: int, mode: str) -> "jdamd.Decoder":
    dec = _decoders.get((index, mode))
    if dec is None:
        layout, channels = MODES[mode]
        dec = jdamd.Decoder(index, layout=layout, channels=channels)
        _decoders[(index, mode)] = dec
    return dec


def decode_jpeg(input: Union[torch.Tensor, Sequence[torch.Tensor]], device="cuda", mode: str = "RGB"):
    """input: a 1-D uint8 CPU tensor holding a JPEG file, or a list of them.  Returns a uint8 tensor
    [3, H, W] (mode "RGB") or [1, H, W] ("GRAY") on `device`, or a list of them.  "GRAY" is the
    JPEG's own luma (include/jd.h JD_FLAG_OUT_GRAY).  Raises ValueError for a bad argument and
    RuntimeError when no GPU is present or an image does not decode (naming its index); nothing is
    returned for a batch with a bad image."""
    single = isinstance(input, torch.Tensor)
    if not single and not isinstance(input, (list, tuple)):
        raise ValueError(f"input: expected a tensor or a list of tensors, not {type(input).__name__}")
    tensors: List[torch.Tensor] = [input] if single else list(input)
    if mode not in MODES:
        raise ValueError(f"mode: one of {tuple(MODES)}, not {mode!r}")
    if not tensors:
        raise ValueError("input: empty list")
    for i, t in enumerate(tensors):
        _check_input(t, "input" if single else f"input[{i}]")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device: a GPU device (\"cuda\", \"cuda:N\"), not {device!r}: this decoder has no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("jdamd.torchio.decode_jpeg: no GPU is available to torch")
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    dev = torch.device("cuda", index)
    dec = _decoder(index, mode)

    tensors = [t.contiguous() for t in tensors]  # (a 1-D view with a stride; contiguous ones are not copied)
    n = len(tensors)
    channels = 1 if mode == "GRAY" else 3
    items = (jdamd._Item * n)()
    results = (jdamd._Result * n)()
    outs: List[torch.Tensor] = []
    hdr = jdamd._Header()
    for i, t in enumerate(tensors):
        # headers here only size the outputs (the batch call parses again and reports per image);
        # an image whose header does not parse gets no output and fails in the batch call
        st = dec.lib.jd_parse(t.data_ptr(), t.numel(), ctypes.byref(hdr))
        if st == jdamd.JD_OK:
            o = torch.empty((channels, hdr.height, hdr.width), dtype=torch.uint8, device=dev)
        else:
            o = None
        outs.append(o)
        items[i] = jdamd._Item(t.data_ptr(), None, t.numel(), o.data_ptr() if o is not None else None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    st = dec.lib.jd_decode_batch(dec.ctx, items, n, results, 1, ctypes.c_void_p(stream))
    if st != jdamd.JD_OK:
        raise RuntimeError("jd_decode_batch: " + jdamd.status_str(st) +
                           (" " + dec.last_error() if st == jdamd.JD_ERR_HIP else ""))
    for i in range(n):
        if results[i].status != jdamd.JD_OK:
            raise RuntimeError(f"decode_jpeg: image {i} did not decode: {jdamd.status_str(results[i].status)}")
    return outs[0] if single else outs
