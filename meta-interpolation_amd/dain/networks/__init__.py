from .DAIN import MetaDAIN

__all__ = (
    "MetaDAIN",
)
