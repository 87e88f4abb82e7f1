"""ESSM — drop-in for rec_pangu/models/multi_task/essm.py:12-75.

Two MLP towers (ctr_layer, cvr_layer: hidden_dim + a Linear to 1, ReLU, dropout) over flatten(emb) only — the dense features
are not used (essm.py:26,48).  task1_pred is pCTR, task2_pred is pCVR, both [B, 1]; the product pCTR * pCVR is what the
loss trains against the conversion label and is not returned.  The xavier pass runs after all modules exist (essm.py:35).
loss(click, conversion, data, weight=0.5) = BCE(conversion, y2) + weight * BCE(click, y1); forward hands it pCTR * pCVR.

HIP path: one gather launch writes the shared [B, ldx] input once and both towers' first Linear read it in place (as in
ShareBottom; their two input gradients meet in a library launch, Fh.fan_out); the towers run through MLP.forward; the two
sigmoids, the product and both BCE terms are ONE launch + its finish (Fh.pair_loss, rp_pair_loss_*).
"""
from typing import Dict, List

from torch import nn

from ... import functional as Fh
from ... import hip
from ..base_model import BaseModel
from ..layers import MLP
from ..utils import get_feature_num


class ESSM(BaseModel):
    def __init__(self, embedding_dim=40, hidden_dim=[128, 64], dropouts=[0.2, 0.2], enc_dict=None, device=None):
        super(ESSM, self).__init__(enc_dict, embedding_dim)
        self.enc_dict = enc_dict
        self.hidden_dim = hidden_dim
        self.dropouts = dropouts
        self.num_sparse_fea, self.num_dense_fea = get_feature_num(self.enc_dict)
        hidden_size = self.num_sparse_fea * self.embedding_dim
        self.ctr_layer = MLP(input_dim=hidden_size, output_dim=1, hidden_units=self.hidden_dim,
                             hidden_activations='relu', dropout_rates=self.dropouts)
        self.cvr_layer = MLP(input_dim=hidden_size, output_dim=1, hidden_units=self.hidden_dim,
                             hidden_activations='relu', dropout_rates=self.dropouts)
        self.sigmoid = nn.Sigmoid()
        self.apply(self._init_weights)

    def forward(self, data, is_training=True):
        if self.on_hip:
            return self._forward_hip(data, is_training)
        hidden = self.embedding_layer(data).flatten(start_dim=1)
        click = self.sigmoid(self.ctr_layer(hidden))
        conversion = self.sigmoid(self.cvr_layer(hidden))
        output_dict = {'task1_pred': click, 'task2_pred': conversion}
        if is_training:
            output_dict['loss'] = self.loss(click, click * conversion, data)
        return output_dict

    def _forward_hip(self, data, is_training):
        x, _ = self.embedding_layer.gather_concat(data, [], want_fm=False)
        x1, x2 = Fh.fan_out(x, 2)
        z1, z2 = self.ctr_layer(x1), self.cvr_layer(x2)  # logits [B, 1]
        if not is_training:
            return {'task1_pred': Fh.sigmoid_sum([z1]), 'task2_pred': Fh.sigmoid_sum([z2])}
        click, conversion, loss = Fh.pair_loss(z1, z2, data['task1_label'].float(), data['task2_label'].float(),
                                               hip.PAIR_ESSM, 0.5, apply_sigmoid=True)
        return {'task1_pred': click, 'task2_pred': conversion, 'loss': loss}

    def loss(self, click, conversion, data, weight=0.5):
        if click.is_cuda:
            # `conversion` is the product pCTR * pCVR (as forward passes it): the kernel takes the factors, so this entry —
            # for callers with probabilities of their own — composes the two terms from the per-task launches
            y1, y2 = data['task1_label'].float(), data['task2_label'].float()
            return Fh.sigmoid_bce_multi([conversion, click], [y2, y1], [1.0, float(weight)], apply_sigmoid=False)[1]
        ctr_loss = nn.functional.binary_cross_entropy(click.squeeze(-1), data['task1_label'])
        cvr_loss = nn.functional.binary_cross_entropy(conversion.squeeze(-1), data['task2_label'])
        return cvr_loss + weight * ctr_loss
