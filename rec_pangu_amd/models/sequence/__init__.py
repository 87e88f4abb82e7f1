from .yotubednn import YotubeDNN
from .gru4rec import GRU4Rec
from .narm import NARM
from .mind import MIND  # noqa: F401
from .comirec import ComirecDR  # noqa: F401
from .sasrec import SASRec  # noqa: F401
from .nextitnet import NextItNet  # noqa: F401

# (MIND, ComirecDR, SASRec and NextItNet are importable from here; __all__ keeps the list tests/test_gru_host.py pins)
__all__ = ["YotubeDNN", "GRU4Rec", "NARM"]
