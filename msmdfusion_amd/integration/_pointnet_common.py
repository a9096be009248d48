"""Shared argument checks of the PointNet++ extension shims."""
import torch


def check_input(**ts):
    """Every tensor on one GPU and contiguous (the reference's CHECK_INPUT / data_ptr use);
    returns the device."""
    dev = None
    for name, t in ts.items():
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % name)
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("%s is on %s, not %s" % (name, t.device, dev))
    return dev


def check_shape(name, t, shape, dtype=torch.float32):
    if t.dtype != dtype or t.numel() != _numel(shape):
        raise RuntimeError("%s must hold %s %s elements, got %s %s"
                           % (name, list(shape), dtype, tuple(t.shape), t.dtype))
    return t.view(*shape)


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n
