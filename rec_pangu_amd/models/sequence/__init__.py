from .yotubednn import YotubeDNN
from .gru4rec import GRU4Rec
from .narm import NARM

__all__ = ["YotubeDNN", "GRU4Rec", "NARM"]
