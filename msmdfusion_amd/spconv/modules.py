"""SparseModule / SparseSequential / ToDense.

Contract taken from the call sites (the legacy twin is
mmdet3d/ops/spconv/modules.py:125-137): a SparseSequential runs its children in
registration order; children that are SparseModules receive the
SparseConvTensor itself, any other nn.Module sees only `.features` -- and is
skipped altogether when the tensor has no active voxel.  Children built from
positional arguments are named "0", "1", ... (make_sparse_convmodule's
checkpoint keys `...0.weight`, `...1.running_mean` depend on it).

The container does not interpret its children one call at a time: the child
list is compiled once into a short program of steps (sparse call / fused
BatchNorm1d(+ReLU) / plain feature op), recompiled only when a child is added
or replaced, and forward() just runs the program.
"""
from torch import nn

from .core import SparseConvTensor


class SparseModule(nn.Module):
    """Marker base: subclasses take a SparseConvTensor inside SparseSequential."""

    def __init__(self, name=None):
        super().__init__()
        self.name = name
        self._sparse_unique_name = ""


def is_spconv_module(module):
    return isinstance(module, SparseModule)


_SPARSE, _BN, _DENSE_OP = 0, 1, 2


def wants_batch_stats(norm):
    """Will this norm layer normalise with the statistics of the batch it is given?  (torch:
    training mode, or no running buffers.)  Only then are the per-tile sums a conv kernel can
    leave behind (SparseConvolution.emit_bn_stats) of any use."""
    return isinstance(norm, nn.BatchNorm1d) and (norm.training or norm.running_mean is None)


class SparseSequential(SparseModule):

    def __init__(self, *children, **named_children):
        super().__init__()
        self._program = None
        self._density = {}
        if len(children) == 1 and isinstance(children[0], dict):
            named_children = dict(children[0], **named_children)
            children = ()
        for position, child in enumerate(children):
            self.add_module(str(position), child)
        for key, child in named_children.items():
            if key in self._modules:
                raise ValueError(f"child name {key!r} is already taken")
            self.add_module(key, child)

    # -- container protocol ------------------------------------------------------
    def add_module(self, name, module):
        super().add_module(name, module)
        self._program = None          # stale: recompile at the next forward

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError(f"child name {name!r} is already taken")
        self.add_module(name, module)

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if isinstance(value, nn.Module):
            self.__dict__["_program"] = None

    def __len__(self):
        return len(self._modules)

    def __iter__(self):
        return iter(self._modules.values())

    def __getitem__(self, position):
        children = tuple(self._modules.values())
        if isinstance(position, slice):
            return SparseSequential(dict(tuple(self._modules.items())[position]))
        if not -len(children) <= position < len(children):
            raise IndexError(f"child index {position} out of range for {len(children)} children")
        return children[position]

    @property
    def sparity_dict(self):
        """name -> fraction of active sites seen by each sparse child at the last
        forward (the reference spells it this way)."""
        return self._density

    # -- execution -----------------------------------------------------------------
    def _compile(self):
        """[(kind, name, module, fuse_relu)]; a BatchNorm1d directly followed by a
        ReLU becomes one fused step (csrc/bn.hip: statistics + apply in two passes)."""
        items = list(self._modules.items())
        steps, skip = [], False
        for pos, (name, child) in enumerate(items):
            if skip:
                skip = False
                continue
            if is_spconv_module(child):
                # conv directly in front of a BatchNorm1d: its kernel can leave the BN's sums
                # (decided at every forward from the norm's mode: slot 3 carries the norm)
                follows = items[pos + 1][1] if pos + 1 < len(items) else None
                steps.append((_SPARSE, name, child,
                              follows if hasattr(child, "weight")
                              and isinstance(follows, nn.BatchNorm1d) else False))
            elif isinstance(child, nn.BatchNorm1d):
                follows = items[pos + 1][1] if pos + 1 < len(items) else None
                skip = isinstance(follows, nn.ReLU)
                steps.append((_BN, name, child, skip))
            else:
                steps.append((_DENSE_OP, name, child, False))
        self.__dict__["_program"] = steps
        for kind, _, child, norm in steps:      # (as of now; forward() re-decides by the mode)
            if kind == _SPARSE and hasattr(child, "weight"):
                child.emit_bn_stats = norm is not False and wants_batch_stats(norm)
        return steps

    def forward(self, x):
        from .functional import bn_act
        steps = self._program
        if steps is None or sum(1 + (s[0] == _BN and bool(s[3])) for s in steps) != \
                len(self._modules):
            steps = self._compile()
        for kind, name, child, fuse_relu in steps:
            if kind == _SPARSE:
                assert isinstance(x, SparseConvTensor), "sparse child needs a SparseConvTensor"
                if hasattr(child, "weight"):     # (slot 3 of a sparse step: the norm behind it)
                    child.emit_bn_stats = fuse_relu is not False and wants_batch_stats(fuse_relu)
                self._density[name] = x.sparity
                x = child(x)
            elif not isinstance(x, SparseConvTensor):
                x = child(x)              # a ToDense() earlier in the chain: plain tensors now
                if fuse_relu:
                    x = nn.functional.relu(x)
            elif x.indices.shape[0]:      # feature-only children are skipped on empty tensors
                if kind == _BN:
                    x = x.replace_feature(bn_act(x.features, child, relu=fuse_relu,
                                                 stats=getattr(x, "bn_stats", None)))
                else:
                    x = x.replace_feature(child(x.features))
        return x


class ToDense(SparseModule):
    def forward(self, x: SparseConvTensor):
        return x.dense()


def sparse_convs(block):
    """The SparseConvolution layers of a block -- and its SparseMaxPool layers, whose
    rulebooks the index pass builds too (SparseConvTensor.plan) -- in call order.  The index
    pass asks for this list for every block of every step; the module tree does not change
    between steps, so the walk (nn.Module.modules(): ~40 us per block, 25 blocks)
    is done once per block object."""
    from .conv import SparseConvolution
    from .pool import SparseMaxPool
    cached = block.__dict__.get("_msmd_sparse_convs")
    if cached is None:
        cached = [m for m in block.modules() if isinstance(m, (SparseConvolution, SparseMaxPool))]
        block.__dict__["_msmd_sparse_convs"] = cached
    return cached
