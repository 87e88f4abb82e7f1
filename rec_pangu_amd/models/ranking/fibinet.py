"""FiBiNet — drop-in for rec_pangu/models/ranking/fibinet.py:13-77.

logit = LR_Layer(data) + MLP(cat(flatten(cat(bilinear(emb), bilinear(senet(emb)), dim=1)), dense)): the SENET reweights the
field embeddings by A = relu(W2 relu(W1 mean_d emb)), and one BilinearInteractionLayer ("field_interaction": a [D, D] matrix per
field pair) is applied to both.  A is a scalar per (sample, field), so the second branch is A_i A_j times the first.  HIP
forward = the wide part's launches -> 1 gather launch -> the SENET, both branches and the cat with the dense columns as ONE
launch that writes the MLP's input (functional.senet_bilinear) -> the MLP GEMMs -> 1 loss launch; the backward of the block is
a sample-major and a pair-major launch per 16384 samples and a finishing one, its dx going straight into the gather's
backward.  Nothing in the step is an ATen kernel, so it replays as a launch plan.
"""
from typing import Dict, List

import torch

from ... import functional as Fh
from ..base_model import BaseModel, build_loss
from ..layers import LR_Layer, MLP, BilinearInteractionLayer, SENET_Layer
from ..utils import get_feature_num, get_linear_input


class FiBiNet(BaseModel):
    def __init__(self, embedding_dim: int = 32, hidden_units: List[int] = [64, 64, 64],
                 loss_fun: str = 'torch.nn.BCELoss()', enc_dict: Dict[str, dict] = None):
        super(FiBiNet, self).__init__(enc_dict, embedding_dim)
        self.hidden_units = hidden_units
        self.loss_fun = build_loss(loss_fun)
        self.enc_dict = enc_dict
        self.num_sparse, self.num_dense = get_feature_num(self.enc_dict)
        self.lr = LR_Layer(enc_dict=self.enc_dict)
        self.senet_layer = SENET_Layer(self.num_sparse, 3)
        self.bilinear_interaction = BilinearInteractionLayer(self.num_sparse, embedding_dim, 'field_interaction')
        input_dim = self.num_sparse * (self.num_sparse - 1) * self.embedding_dim + self.num_dense
        self.dnn = MLP(input_dim=input_dim, output_dim=1, hidden_units=self.hidden_units,
                       hidden_activations='relu', dropout_rates=0)
        self.reset_parameters()

    def hip_supported(self) -> bool:
        from ... import hip
        return hip.bilinear_fits(self.num_sparse, self.embedding_dim, self.senet_layer.excitation[0].weight.shape[0],
                                 self.bilinear_interaction.bilinear_type)

    def forward(self, data, is_training=True):
        F, D = self.num_sparse, self.embedding_dim
        wide_logit = self.lr(data)
        if self.on_hip:
            if self.hip_supported():
                x, _ = self.embedding_layer.gather_concat(data, self._dense_list(data), want_fm=False)
                comb_out = Fh.senet_bilinear(x, F, D, self.senet_layer, self.bilinear_interaction, self.num_dense)
                return self._finish([wide_logit, self.dnn(comb_out)], data, is_training, self.loss_fun)
            from ... import hip
            hip.note_torch_path(f"{type(self).__name__}'s SENET + bilinear interaction over {F} fields, D={D} "
                                "(outside hip.bilinear_fits)")
        feature_emb = self.embedding_layer(data)
        senet_emb = feature_emb * self.senet_layer.weights_A(feature_emb).unsqueeze(-1)
        bilinear_p = self.bilinear_interaction.torch_pairs(feature_emb)
        bilinear_q = self.bilinear_interaction.torch_pairs(senet_emb)
        comb_out = torch.flatten(torch.cat([bilinear_p, bilinear_q], dim=1), start_dim=1)
        comb_out = torch.cat([comb_out, get_linear_input(self.enc_dict, data)], dim=1)
        return self._finish([wide_logit, self.dnn(comb_out)], data, is_training, self.loss_fun)
