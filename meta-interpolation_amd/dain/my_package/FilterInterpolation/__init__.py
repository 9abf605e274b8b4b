from .FilterInterpolationModule import FilterInterpolationModule
from .FilterInterpolationLayer import FilterInterpolationLayer

__all__ = ['FilterInterpolationModule', 'FilterInterpolationLayer']
