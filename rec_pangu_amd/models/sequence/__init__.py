from .yotubednn import YotubeDNN
from .gru4rec import GRU4Rec
from .narm import NARM
from .mind import MIND  # noqa: F401
from .comirec import ComirecDR, ComirecSA  # noqa: F401
from .sasrec import SASRec  # noqa: F401
from .nextitnet import NextItNet  # noqa: F401
from .srgnn import SRGNN  # noqa: F401
from .niser import NISER  # noqa: F401
from .gcsan import GCSAN  # noqa: F401
from .stamp import STAMP  # noqa: F401
from .clrec import CLRec  # noqa: F401
from .contrarec import ContraRec  # noqa: F401

# (MIND, ComirecDR, ComirecSA, SASRec, NextItNet, SRGNN, NISER, GCSAN, STAMP, CLRec and ContraRec are importable from here; __all__ keeps the list tests/test_gru_host.py pins)
__all__ = ["YotubeDNN", "GRU4Rec", "NARM"]
