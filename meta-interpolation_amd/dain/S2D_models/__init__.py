from .S2DF import *
