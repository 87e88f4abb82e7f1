from .deepfm import DeepFM
from .xdeepfm import xDeepFM
from .dcn import DCN
from .autoint import AutoInt
from .fm import FM
from .wdl import WDL
from .nfm import NFM
from .lr import LR
from .masknet import MaskNet
from .aoanet import AOANet
from .ccpm import CCPM
from .fibinet import FiBiNet
from .afm import AFM
from .afn import AFN

__all__ = ["DeepFM", "xDeepFM", "DCN", "AutoInt", "FM", "WDL", "NFM", "LR", "MaskNet", "AOANet", "CCPM", "FiBiNet", "AFM",
           "AFN"]
