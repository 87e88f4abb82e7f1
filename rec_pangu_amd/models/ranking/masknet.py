"""MaskNet — drop-in for rec_pangu/models/ranking/masknet.py:13-87.

x = cat(flatten(emb), dense); v = mean of block_num MaskBlocks over (x, x) (use_parallel) or the blocks chained on their
own output with x as every block's mask input (serial); pred = sigmoid(MLP(v)).  HIP forward = 1 gather launch -> the
whole block stack on one autograd node (5 launches per block: functional.mask_block_stack, which also sums the gradients
the blocks send back to x) -> MLP GEMMs -> 1 loss launch; nothing in the step is an ATen kernel, so it replays as a
launch plan.
"""
from typing import Dict, List

import torch

from ... import functional as Fh
from ..base_model import BaseModel, build_loss
from ..layers import MLP, MaskBlock
from ..utils import get_dnn_input_dim, get_linear_input


class MaskNet(BaseModel):
    def __init__(self, embedding_dim: int = 32, block_num: int = 3, use_parallel: bool = True,
                 reduction_factor: float = 0.3, hidden_units: List[int] = [64, 64, 64],
                 loss_fun: str = 'torch.nn.BCELoss()', enc_dict: Dict[str, dict] = None):
        super(MaskNet, self).__init__(enc_dict, embedding_dim)
        self.loss_fun = build_loss(loss_fun)
        self.enc_dict = enc_dict
        self.block_num = block_num
        self.hidden_units = hidden_units
        self.reduction_factor = reduction_factor
        self.use_parallel = use_parallel
        self.input_dim = get_dnn_input_dim(self.enc_dict, self.embedding_dim)
        self.mask_input_dim = self.block_output_dim = self.input_dim
        self.mask_block_list = torch.nn.ModuleList(
            MaskBlock(self.input_dim, self.mask_input_dim, self.block_output_dim, self.reduction_factor)
            for _ in range(self.block_num))
        self.mlp = MLP(self.block_output_dim, hidden_units=self.hidden_units, output_dim=1)
        self.reset_parameters()

    def forward(self, data, is_training=True):
        if self.on_hip and self.block_num > 0:
            x, _ = self.embedding_layer.gather_concat(data, self._dense_list(data), want_fm=False)
            # v keeps x's zero padding columns; the MLP's first Linear reads its first input_dim columns
            v = Fh.mask_block_stack(x, self.mask_block_list, self.use_parallel)
            return self._finish([self.mlp(v)], data, is_training, self.loss_fun)
        feature_emb = self.embedding_layer(data)
        x = torch.cat([feature_emb.flatten(start_dim=1), get_linear_input(self.enc_dict, data)], dim=1)
        if self.use_parallel:
            v = torch.stack([block(x, x) for block in self.mask_block_list], dim=1).mean(dim=1)
        else:
            v = x
            for block in self.mask_block_list:
                v = block(v, x)
        return self._finish([self.mlp(v)], data, is_training, self.loss_fun)
