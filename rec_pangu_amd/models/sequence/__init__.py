from .yotubednn import YotubeDNN

__all__ = ["YotubeDNN"]
