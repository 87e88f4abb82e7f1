from .activation import Dice, get_activation
from .embedding import EmbeddingLayer
from .deep import MLP
from .shallow import LR_Layer
from .interaction import (InnerProductLayer, FM_Layer, CrossInteractionLayer, CrossNet,
                          CompressedInteractionNet, MaskBlock, GeneralizedInteractionNet,
                          GeneralizedInteraction, BilinearInteractionLayer, SENET_Layer)
from .attention import ScaledDotProductAttention, MultiHeadAttention, MultiHeadSelfAttention
from .sequence import MaskedAveragePooling, MaskedSumPooling, KMaxPooling, GRU4RecEncoder, STAMPLayer, BERT4RecEncoder
from .multi_interest import CapsuleNetwork, MultiInterestSelfAttention
from .transformer import FeedForward, TransformerLayer, TransformerEncoder
from .conv import NextItNetLayer, ResBlockOneMasked, ResBlockTwoMasked, MaskedConv1d, LayerNorm
from .graph import SRGNNConv, SRGNNCell

__all__ = ["Dice", "get_activation", "EmbeddingLayer", "MLP", "LR_Layer", "InnerProductLayer", "FM_Layer",
           "CrossInteractionLayer", "CrossNet", "CompressedInteractionNet", "MaskBlock", "GeneralizedInteractionNet",
           "GeneralizedInteraction", "BilinearInteractionLayer", "SENET_Layer", "ScaledDotProductAttention",
           "MultiHeadAttention", "MultiHeadSelfAttention", "MaskedAveragePooling", "MaskedSumPooling", "KMaxPooling",
           "GRU4RecEncoder", "CapsuleNetwork", "FeedForward", "TransformerLayer", "TransformerEncoder", "NextItNetLayer",
           "ResBlockOneMasked", "ResBlockTwoMasked", "MaskedConv1d", "LayerNorm", "SRGNNConv", "SRGNNCell", "STAMPLayer",
           "MultiInterestSelfAttention", "BERT4RecEncoder"]
