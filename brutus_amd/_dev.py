"""The three helpers every module that calls the library shares: torch with a GPU behind it,
the current stream as the integer `void *stream` takes, and a host array's device copy."""
import numpy as np

from . import _lib


def _torch(only="the grid likelihood only runs on the HIP path, there is no CPU fallback."):
    import torch
    if not torch.cuda.is_available():
        raise _lib.BrutusError(
            "brutus_amd: no GPU visible (torch.cuda.is_available() is False); " + only)
    return torch


def _stream_ptr(torch):
    return torch.cuda.current_stream().cuda_stream


def to_device(a, dtype, dev):
    """`a` as a C-contiguous array of `dtype`, copied to device `dev`: what a `d_` parameter of
    that element type takes.  A tensor (the device form of `pdf.los_tables`) stays where it is:
    on `dev` with that element type it is handed on as it is, never copied through the host."""
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.from_numpy(np.empty(0, dtype=dtype)).dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
