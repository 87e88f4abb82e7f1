"""AITM — drop-in for rec_pangu/models/multi_task/aitm.py:14-100.

click_tower / conversion_tower (MLP without an output layer) over flatten(emb); info_layer (Linear + ReLU + Dropout) carries
the click tower's representation to the conversion task; attention_layer = MultiHeadSelfAttention(tower_dims[-1]) runs over
the T = 2 tokens [conversion tower, info] (one head as wide as the tower: no W_res) and its output is summed over the tokens;
click_layer / conversion_layer are Linear(., 1) + Sigmoid.  Predictions are [B] (squeezed on dim 1).  There is no `device`
argument.  loss = BCE(p1, y1) + BCE(p2, y2) + constraint_weight * sum_b max(p2 - p1, 0): the constraint is a SUM over the
batch (aitm.py:97).

HIP path: one gather launch, both towers read its [B, ldx] output in place (Fh.fan_out sums their input gradients with a
library launch, as it does for the click tower's two consumers); the two tokens are packed into one [B, 2, a] buffer
(Fh.stack_tokens); the attention is one projection GEMM over the B*2 token rows + the wide-head core with the token sum fused
in (MultiHeadAttention.self_attention_sum -> Fh.attention_wide); the two sigmoids, both BCE terms and the constraint are one
launch + its finish (Fh.pair_loss).
"""
from typing import Dict, List

import torch
from torch import nn

from ... import functional as Fh
from ... import hip
from ..base_model import BaseModel
from ..layers import MLP, MultiHeadSelfAttention
from ..utils import get_feature_num


class AITM(BaseModel):
    def __init__(self, embedding_dim: int = 32, tower_dims: List[int] = [400, 400, 400],
                 drop_prob: List[float] = [0.1, 0.1, 0.1], enc_dict: Dict[str, dict] = None):
        super(AITM, self).__init__(enc_dict, embedding_dim)
        self.enc_dict = enc_dict
        self.tower_dims = tower_dims
        self.drop_prob = drop_prob
        self.num_sparse_fea, self.num_dense_fea = get_feature_num(self.enc_dict)
        self.tower_input_size = self.num_sparse_fea * self.embedding_dim
        self.click_tower = MLP(input_dim=self.tower_input_size, hidden_units=self.tower_dims,
                               hidden_activations='relu', dropout_rates=self.drop_prob)
        self.conversion_tower = MLP(input_dim=self.tower_input_size, hidden_units=self.tower_dims,
                                    hidden_activations='relu', dropout_rates=self.drop_prob)
        self.attention_layer = MultiHeadSelfAttention(self.tower_dims[-1])
        self.info_layer = nn.Sequential(nn.Linear(tower_dims[-1], tower_dims[-1]), nn.ReLU(), nn.Dropout(drop_prob[-1]))
        self.click_layer = nn.Sequential(nn.Linear(tower_dims[-1], 1), nn.Sigmoid())
        self.conversion_layer = nn.Sequential(nn.Linear(tower_dims[-1], 1), nn.Sigmoid())
        self.apply(self._init_weights)

    def forward(self, data, is_training=True):
        if self.on_hip:
            return self._forward_hip(data, is_training)
        feature_embedding = self.embedding_layer(data).flatten(start_dim=1)
        tower_click = self.click_tower(feature_embedding)
        tower_conversion = torch.unsqueeze(self.conversion_tower(feature_embedding), 1)
        info = torch.unsqueeze(self.info_layer(tower_click), 1)
        ait = self.attention_layer(torch.cat([tower_conversion, info], 1))
        ait = torch.sum(ait, dim=1)
        click = torch.squeeze(self.click_layer(tower_click), dim=1)
        conversion = torch.squeeze(self.conversion_layer(ait), dim=1)
        output_dict = {'task1_pred': click, 'task2_pred': conversion}
        if is_training:
            output_dict['loss'] = self.loss(data['task1_label'], click, data['task2_label'], conversion)
        return output_dict

    def _forward_hip(self, data, is_training):
        x, _ = self.embedding_layer.gather_concat(data, [], want_fm=False)
        x1, x2 = Fh.fan_out(x, 2)
        c1, c2 = Fh.fan_out(self.click_tower(x1), 2)  # read by info_layer and by click_layer
        tower_conversion = self.conversion_tower(x2)
        lin, drop = self.info_layer[0], self.info_layer[2]
        info = Fh.linear_act(c1, lin.weight, lin.bias, Fh.ACT_RELU)
        if self.training and 0 < drop.p < 1:
            info = Fh.dropout(info, drop.p)
        elif self.training and drop.p >= 1:
            info = drop(info)
        ait = self.attention_layer.self_attention_sum(Fh.stack_tokens([tower_conversion, info]))  # [B, a]
        z1 = Fh.linear_act(c2, self.click_layer[0].weight, self.click_layer[0].bias, Fh.ACT_NONE).squeeze(1)
        z2 = Fh.linear_act(ait, self.conversion_layer[0].weight, self.conversion_layer[0].bias, Fh.ACT_NONE).squeeze(1)
        if not is_training:
            return {'task1_pred': Fh.sigmoid_sum([z1]).squeeze(1), 'task2_pred': Fh.sigmoid_sum([z2]).squeeze(1)}
        click, conversion, loss = Fh.pair_loss(z1, z2, data['task1_label'].float(), data['task2_label'].float(),
                                               hip.PAIR_AITM, 0.6, apply_sigmoid=True)
        return {'task1_pred': click, 'task2_pred': conversion, 'loss': loss}

    def loss(self, click_label, click_pred, conversion_label, conversion_pred, constraint_weight=0.6):
        if click_pred.is_cuda:
            return Fh.pair_loss(click_pred, conversion_pred, click_label.float(), conversion_label.float(), hip.PAIR_AITM,
                                constraint_weight, apply_sigmoid=False)[2]
        click_loss = nn.functional.binary_cross_entropy(click_pred, click_label)
        conversion_loss = nn.functional.binary_cross_entropy(conversion_pred, conversion_label)
        label_constraint = torch.maximum(conversion_pred - click_pred, torch.zeros_like(click_label))
        constraint_loss = torch.sum(label_constraint)
        return click_loss + conversion_loss + constraint_weight * constraint_loss
