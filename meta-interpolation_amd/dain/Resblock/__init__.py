from .BasicBlock import *
