"""The a-side head's reduce convs split by input-channel half for whole-sequence inference.

head_a_indexed runs, for every (target, reference) pair, the 3x3 reduce conv (2C -> C,
rgbd_segmentation_RAA.py:189-190, :241-242) over cat = [gate(Z_a) | V_a].  A convolution is linear
in its input channels,

    conv(W, [gz | v]) = conv(W[..., :C], gz) + conv(W[..., C:], v),

and the second term depends on the target frame alone: a sequence has T such frames and P = T N
pairs.  Here

* FeatureBank.reduce_partials(model) computes u = conv(W[..., C:], v) once per frame of the bank,
  as the unrounded fp32 accumulator (cn_conv_fwd_partial), for both modalities;
* head_a_indexed(split=True) gates Z_a alone (cn_gate_fwd: no concat, no copy of V_a per pair) and
  runs the half-width conv whose GEMM epilogue adds the a-role frame's rows of u through the pair
  map, then the folded eval-mode BN, then rounds once (cn_conv_fwd_affine_add, gemm.hip EPI 5).

The reduce convs' FLOPs go from 2 P HW C (9 2C) to 2 (P + T) HW C (9 C): (1 + 1/N) / 2 of the
default's.  The sum acc(gz) + acc(v) is the concat conv's accumulator up to the order of the fp32
additions (exactly it on operands whose partial sums are exact: tests/test_gpu_conv_affine_add.py),
and like the folded head it rounds once where the default head rounds the raw conv output first.

model.set_head_split() holds the state below; segment_sequence(head="split") uses it.
"""
import weakref

from . import ops
from .bn_fold import FoldTables


def reduce_sides(model):
    """(reduce conv, its BN) of the two modalities, in head_a_indexed's order."""
    return ((model.reduce_channels_A, model.bn_A), (model.depth_reduce_channels, model.depth_bn))


class HeadSplit:
    """A model's split-head state (model.set_head_split): the two contiguous halves of each reduce
    conv weight in the compute dtype (ops.HCACHE: WCACHE's staleness rule) and the folded
    (scale, shift) tables of bn_A / depth_bn -- those of the active BN-fold state
    (model.bn_fold.head, or model.fp8_static.head under fold_bn), else tables of its own under
    FoldTables' staleness rule."""

    def __init__(self, model):
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError("set_head_split: the model must be on the GPU")
        self.model = weakref.ref(model)
        self._own = None
        self.tables()
        for reduce, _ in reduce_sides(model):
            self.halves(reduce, model.compute_dtype)

    def tables(self):
        """The FoldTables holding bn_A and depth_bn."""
        m = self.model()
        fold = getattr(m, "bn_fold", None)
        if fold is None and getattr(getattr(m, "fp8_static", None), "head", None) is not None:
            fold = m.fp8_static
        if fold is not None:
            return fold.head
        if self._own is None:
            self._own = FoldTables(m, modules=[("bn_A", m.bn_A), ("depth_bn", m.depth_bn)])
        return self._own

    @staticmethod
    def halves(reduce, dtype):
        """(W[..., :C] for the gated half, W[..., C:] for the pass-through half) of one reduce conv,
        each [Cout][9 C] in `dtype`, current with the weight."""
        return ops.HCACHE.get(reduce.weight, dtype)
