"""SparseMaxPool / SparseMaxPool3d: the module of mmdet3d/ops/spconv/pool.py:21-87 on the HIP
max-pool kernels (csrc/pool.hip).

Kept: constructor arguments and defaults (stride=1, padding=0, dilation=1), output shape
rule (get_conv_output_size), the rulebook (the strided conv rulebook of the same geometry,
ops.get_indice_pairs with transpose=0 -- here the SAME object the equal conv would use,
through SparseConvTensor.cached_rulebook) and the functors' arithmetic (src/maxpool.cc:20-62):
the output starts at zero, an input replaces it only when out < in, and the gradient reaches
every input equal to its output.  Added as in spconv-2.x: a keyword `indice_key`, so that a
SparseInverseConv3d can pair with the pool; `algo` is accepted and ignored.  SubM pooling is
not built.
"""
from torch.autograd import Function

from .. import kernels as K
from .conv import expand_nd
from .core import SparseConvTensor
from .modules import SparseModule


class _MaxPoolFunction(Function):

    @staticmethod
    def forward(ctx, features, nbr_bwd, n_out):
        out = K.maxpool_fwd(features, nbr_bwd, n_out)
        ctx.save_for_backward(features, out, nbr_bwd)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        features, out, nbr_bwd = ctx.saved_tensors
        return K.maxpool_bwd(features, out, grad_out.contiguous(), nbr_bwd), None, None


def indice_maxpool(features, rb):
    """Max-pool `features` (the rulebook's input rows) over rulebook `rb` -> [rb.n_out, C]."""
    rb.check_ready()
    if rb.nbr_bwd is None:
        raise RuntimeError("max-pool needs the rulebook's input-side table (nbr_bwd)")
    return _MaxPoolFunction.apply(features, rb.nbr_bwd, rb.n_out)


class SparseMaxPool(SparseModule):
    is_pool = True
    # (what the index pass asks of every sparse layer: a pool is a strided, set-changing layer)
    transposed = inverse = conv1x1 = False

    def __init__(self, ndim, kernel_size, stride=1, padding=0, dilation=1, subm=False,
                 indice_key=None, algo=None, name=None):
        super().__init__(name=name)
        if ndim != 3:
            raise NotImplementedError("only 3-D sparse max-pooling is built")
        if subm:
            raise NotImplementedError("SubM max-pooling is not built")
        self.ndim = ndim
        self.kernel_size = expand_nd(ndim, kernel_size)
        self.stride = expand_nd(ndim, stride)
        self.padding = expand_nd(ndim, padding)
        self.dilation = expand_nd(ndim, dilation)
        self.subm = subm
        self.indice_key = indice_key
        self.algo = algo

    def extra_repr(self):
        return "kernel_size={kernel_size}, stride={stride}, padding={padding}".format(
            **self.__dict__)

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        out_spatial_shape = K.conv_output_size(input.spatial_shape, self.kernel_size, self.stride,
                                               self.padding, self.dilation)
        indice_dict = input.indice_dict.copy()
        if self.indice_key is not None:
            msg = f"your indice key {self.indice_key} already exists in this sparse tensor."
            assert self.indice_key not in indice_dict, msg
        rb = input.cached_rulebook(self.kernel_size, self.stride, self.padding, self.dilation,
                                   False)
        if self.indice_key is not None:
            indice_dict[self.indice_key] = rb
        out_features = indice_maxpool(input.features, rb)
        out_tensor = input.shadow_copy()
        out_tensor.indices = rb.out_indices
        out_tensor = out_tensor.replace_feature(out_features)
        out_tensor.indice_dict = indice_dict
        out_tensor.spatial_shape = out_spatial_shape
        return out_tensor


class SparseMaxPool3d(SparseMaxPool):

    def __init__(self, kernel_size, stride=1, padding=0, dilation=1, indice_key=None, algo=None,
                 name=None):
        super().__init__(3, kernel_size, stride, padding, dilation, indice_key=indice_key,
                         algo=algo, name=name)
