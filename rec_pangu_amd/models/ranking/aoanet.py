"""AOANet — drop-in for rec_pangu/models/ranking/aoanet.py:14-115.

pred = sigmoid(fc(cat(MLP(cat(flatten(emb), dense)), flatten(GIN(emb))))): an MLP trunk without an output layer beside the
generalized interaction net, one Linear over both.  HIP forward = 1 gather launch -> the GIN on one autograd node reading the
embedding columns of the MLP input buffer in place (functional.gin_stack: one launch per layer, no outer product) -> the MLP
GEMMs -> fc as two GEMV launches on the halves of its weight -> 1 loss launch that adds the two logits; nothing in the step
is an ATen kernel, so it replays as a launch plan.
"""
from typing import Dict, List

import torch
from torch import nn

from ... import functional as Fh
from ..base_model import BaseModel, build_loss
from ..layers import MLP, GeneralizedInteractionNet
from ..utils import get_feature_num, get_linear_input


class AOANet(BaseModel):
    def __init__(self, embedding_dim: int = 32, dnn_hidden_units: List[int] = [64, 64, 64],
                 num_interaction_layers: int = 3, num_subspaces: int = 4, loss_fun: str = 'torch.nn.BCELoss()',
                 enc_dict: Dict[str, dict] = None):
        super(AOANet, self).__init__(enc_dict, embedding_dim)
        self.dnn_hidden_units = dnn_hidden_units
        self.loss_fun = build_loss(loss_fun)
        self.enc_dict = enc_dict
        self.num_sparse, self.num_dense = get_feature_num(self.enc_dict)
        self.dnn = MLP(input_dim=self.embedding_dim * self.num_sparse + self.num_dense, output_dim=None,
                       hidden_units=self.dnn_hidden_units)
        self.gin = GeneralizedInteractionNet(num_interaction_layers, num_subspaces, self.num_sparse, self.embedding_dim)
        self.fc = nn.Linear(dnn_hidden_units[-1] + num_subspaces * self.embedding_dim, 1)
        self.reset_parameters()

    def forward(self, data, is_training=True):
        if self.on_hip and self.gin.hip_supported():
            x, _ = self.embedding_layer.gather_concat(data, self._dense_list(data), want_fm=False)
            n = self.num_sparse * self.embedding_dim
            link = getattr(self.embedding_layer, "_fm_link", None)
            aliased = link is not None and x.requires_grad and torch.is_grad_enabled()
            # the embedding block of the MLP input buffer as the GIN's rows (no copy: the kernels take the row stride); its
            # gradient joins the MLP's dX inside the gather's backward (Fh.token_alias)
            rows = Fh.token_alias(x, n, link) if aliased else x[:, :n]
            interact_out = Fh.gin_stack(rows, self.num_sparse, self.embedding_dim, self.gin.layers)  # [B, O D]
            dnn_out = self.dnn(x, fm_link=link if aliased else None)
            # fc over the concatenation = the sum of two products with the halves of its weight (no cat, no slice node)
            w_dnn, w_gin = Fh.row_split(self.fc.weight, self.dnn_hidden_units[-1])
            logits = [Fh.linear_act(dnn_out, w_dnn, self.fc.bias), Fh.linear_act(interact_out, w_gin, None)]
            return self._finish(logits, data, is_training, self.loss_fun)
        feature_emb = self.embedding_layer(data)
        dense_input = get_linear_input(self.enc_dict, data)
        dnn_out = self.dnn(torch.cat([feature_emb.flatten(start_dim=1), dense_input], dim=1))
        interact_out = self.gin(feature_emb).flatten(start_dim=1)
        y_pred = self.fc(torch.cat([dnn_out, interact_out], dim=-1))
        return self._finish([y_pred], data, is_training, self.loss_fun)
