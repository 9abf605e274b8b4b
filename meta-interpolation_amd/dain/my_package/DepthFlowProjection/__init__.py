from .DepthFlowProjectionModule import DepthFlowProjectionModule
from .DepthFlowProjectionLayer import DepthFlowProjectionLayer

__all__ = ['DepthFlowProjectionModule', 'DepthFlowProjectionLayer']
