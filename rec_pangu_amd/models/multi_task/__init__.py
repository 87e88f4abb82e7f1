from .mmoe import MMOE
from .omoe import OMOE
from .mlmmoe import MLMMOE
from .sharebottom import ShareBottom
from .essm import ESSM
from .aitm import AITM

__all__ = ["MMOE", "OMOE", "MLMMOE", "ShareBottom", "ESSM", "AITM"]
