"""AFN — drop-in for rec_pangu/models/ranking/afn.py:14-102.

afn_out = dense_layer(flatten(exp_batch_norm(exp(coefficient_W log_batch_norm(log max(|emb|, 1e-5)))))): every field embedding
goes through a logarithm, L "logarithmic neurons" take weighted sums over the fields per embedding column (products of
powers of the fields), and the two BatchNorm1d take their statistics over batch and column (channel = field, then neuron).
With ensemble_dnn a second, independent EmbeddingLayer feeds a plain MLP and y = sigmoid(fc(cat[afn_out, dnn_out])); the
dense features are not used (afn.py:74-80).  Both MLPs keep the reference's default dropout of 0.1.

HIP forward = 1 gather launch -> the logarithmic net with both BatchNorms as ONE autograd node that reads the gather's rows
in place and writes dense_layer's input (functional.logarithmic_net, csrc/lognet.hip) -> the MLP GEMMs; the second layer's
gather -> its MLP; fc without the cat (functional.pair_fc) -> 1 loss launch.  The block's dx goes straight into the gather's
backward.  Nothing in the step is an ATen kernel, so it replays as a launch plan.
"""
from typing import Dict, List

import torch
from torch import nn

from ... import functional as Fh
from ..base_model import BaseModel, build_loss
from ..layers import MLP
from ..layers.embedding import EmbeddingLayer, make_embedding_layer
from ..utils import get_feature_num


class AFN(BaseModel):
    def __init__(self, embedding_dim: int = 32, dnn_hidden_units: List[int] = [64, 64, 64],
                 afn_hidden_units: List[int] = [64, 64, 64], ensemble_dnn: bool = True,
                 loss_fun: str = 'torch.nn.BCELoss()', logarithmic_neurons: int = 5, enc_dict: Dict[str, dict] = None):
        super(AFN, self).__init__(enc_dict, embedding_dim)
        self.dnn_hidden_units = dnn_hidden_units
        self.afn_hidden_units = afn_hidden_units
        self.loss_fun = build_loss(loss_fun)
        self.enc_dict = enc_dict
        self.num_sparse, self.num_dense = get_feature_num(self.enc_dict)
        self.coefficient_W = nn.Linear(self.num_sparse, logarithmic_neurons, bias=False)
        self.dense_layer = MLP(input_dim=embedding_dim * logarithmic_neurons, output_dim=1,
                               hidden_units=afn_hidden_units, use_bias=True)
        self.log_batch_norm = nn.BatchNorm1d(self.num_sparse)
        self.exp_batch_norm = nn.BatchNorm1d(logarithmic_neurons)
        self.ensemble_dnn = ensemble_dnn
        if ensemble_dnn:
            self.embedding_layer2 = make_embedding_layer(self.enc_dict, self.embedding_dim)
            self.dnn = MLP(input_dim=embedding_dim * self.num_sparse, output_dim=1, hidden_units=dnn_hidden_units,
                           use_bias=True)
            self.fc = nn.Linear(2, 1)
        self.reset_parameters()

    def hip_supported(self) -> bool:
        from ... import hip
        layers = [self.embedding_layer] + ([self.embedding_layer2] if self.ensemble_dnn else [])
        return (all(type(m) is EmbeddingLayer for m in layers)
                and all(type(bn) is nn.BatchNorm1d for bn in (self.log_batch_norm, self.exp_batch_norm))
                and self.log_batch_norm.training == self.exp_batch_norm.training
                and hip.lognet_fits(self.num_sparse, self.embedding_dim, self.coefficient_W.out_features))

    def forward(self, data, is_training=True):
        F, D = self.num_sparse, self.embedding_dim
        if self.on_hip and self.hip_supported():
            x, _ = self.embedding_layer.gather_concat(data, [], want_fm=False)
            dnn_input = Fh.logarithmic_net(x, F, D, self.coefficient_W, self.log_batch_norm, self.exp_batch_norm)
            afn_out = self.dense_layer(dnn_input)
            if not self.ensemble_dnn:
                return self._finish([afn_out], data, is_training, self.loss_fun)
            x2, _ = self.embedding_layer2.gather_concat(data, [], want_fm=False)
            return self._finish([Fh.pair_fc(afn_out, self.dnn(x2), self.fc)], data, is_training, self.loss_fun)
        if self.on_hip:
            from ... import hip
            hip.note_torch_path(f"{type(self).__name__}'s logarithmic net over {F} fields, D={D}, "
                                f"{self.coefficient_W.out_features} neurons (outside hip.lognet_fits, or row-sharded tables)")
        afn_out = self.dense_layer(self.logarithmic_net(self.embedding_layer(data)))
        if self.ensemble_dnn:
            dnn_out = self.dnn(self.embedding_layer2(data).flatten(start_dim=1))
            y_pred = self.fc(torch.cat([afn_out, dnn_out], dim=-1))
        else:
            y_pred = afn_out
        return self._finish([y_pred], data, is_training, self.loss_fun)

    def logarithmic_net(self, feature_emb):
        """afn.py:93-102 on torch ops (the CPU path, and the HIP device outside hip.lognet_fits)"""
        log_emb = torch.log(torch.clamp(torch.abs(feature_emb), min=1e-5))
        log_emb = self.log_batch_norm(log_emb)  # [B, F, D]: channel = field
        logarithmic_out = self.coefficient_W(log_emb.transpose(2, 1)).transpose(1, 2)
        cross_out = self.exp_batch_norm(torch.exp(logarithmic_out))  # [B, L, D]: channel = neuron
        return torch.flatten(cross_out, start_dim=1)
