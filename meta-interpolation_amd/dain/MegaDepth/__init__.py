from .MegaDepth_model import *
