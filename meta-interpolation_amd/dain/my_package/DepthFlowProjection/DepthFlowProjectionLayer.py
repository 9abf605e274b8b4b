"""DAIN's depth-aware flow projection on the gfx950 kernels (csrc/dainwarp.hip through hip_ops.depth_flow_projection).

Same call surface as the reference's dain/my_package/DepthFlowProjection/DepthFlowProjectionLayer.py:
``apply(input1, input2, requires_grad)`` with ``fillhole = not requires_grad`` (:19).  Device tensors only: a CPU tensor raises
NotImplementedError.
"""
from .... import hip_ops


class DepthFlowProjectionLayer:
    """``DepthFlowProjectionLayer.apply(input1, input2, requires_grad)``: the flow input1 [B,2,H,W] projected to the intermediate
    frame with the depth inverses input2 [B,1,H,W] as weights; holes are filled when no gradient is wanted."""

    @staticmethod
    def apply(input1, input2, requires_grad):
        return hip_ops.depth_flow_projection(input1, input2, fillhole=not requires_grad)
