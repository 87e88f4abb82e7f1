"""CCPM — drop-in for rec_pangu/models/ranking/ccpm.py:14-107.

pred = sigmoid(fc(flatten(conv stack over the field embeddings))): three [ZeroPad2d -> Conv2d (kh, 1) -> KMaxPooling -> Tanh]
layers along the field axis.  No step of the stack mixes two embedding columns, so the HIP forward is 1 gather launch -> the
whole stack as ONE launch on the embedding columns of the gather's row buffer (functional.ccpm_conv_stack) -> fc as one GEMV
launch -> 1 loss launch; the backward is one stack launch (+ its finishing launch) whose dx goes straight into the gather's
backward.  Nothing in the step is an ATen kernel, so it replays as a launch plan.  Dense features are ignored, as upstream.
"""
from typing import Dict, List

import torch
from torch import nn

from ... import functional as Fh
from ..base_model import BaseModel, build_loss
from ..layers import KMaxPooling, get_activation
from ..utils import get_feature_num


class CCPM(BaseModel):
    def __init__(self, embedding_dim: int = 32, hidden_units: List[int] = [64, 64, 64], channels: List[int] = [4, 4, 2],
                 kernel_heights: List[int] = [6, 5, 3], loss_fun: str = 'torch.nn.BCELoss()',
                 enc_dict: Dict[str, dict] = None):
        super(CCPM, self).__init__(enc_dict, embedding_dim)
        self.dnn_hidden_units = hidden_units  # (accepted and unused, as upstream)
        self.loss_fun = build_loss(loss_fun)
        self.enc_dict = enc_dict
        self.num_sparse, self.num_dense = get_feature_num(self.enc_dict)
        self.conv_layer = CCPM_ConvLayer(self.num_sparse, channels=channels, kernel_heights=kernel_heights)
        conv_out_dim = 3 * embedding_dim * channels[-1]  # 3 is k-max-pooling size of the last layer
        self.fc = nn.Linear(conv_out_dim, 1)
        self.reset_parameters()

    def forward(self, data, is_training=True):
        F, D = self.num_sparse, self.embedding_dim
        if self.on_hip:
            if self.conv_layer.hip_supported(D):
                x, _ = self.embedding_layer.gather_concat(data, [], want_fm=False)
                flatten_out = Fh.ccpm_conv_stack(x, F, D, self.conv_layer)  # [B, C_last 3 D], fc.weight applies unpermuted
                return self._finish([Fh.linear_act(flatten_out, self.fc.weight, self.fc.bias, Fh.ACT_NONE)], data,
                                    is_training, self.loss_fun)
            from ... import hip
            hip.note_torch_path(f"CCPM's conv stack over {F} fields, D={D}, channels {self.conv_layer.channels[1:]} "
                                "(outside hip.ccpm_fits)")
        feature_emb = self.embedding_layer(data)
        conv_out = self.conv_layer.torch_stack(torch.unsqueeze(feature_emb, 1))  # (bs, 1, field, emb) -> (bs, C, 3, emb)
        y_pred = self.fc(torch.flatten(conv_out, start_dim=1))
        return self._finish([y_pred], data, is_training, self.loss_fun)


class CCPM_ConvLayer(nn.Module):
    """Input X: tensor of shape (batch_size, 1, num_fields, embedding_dim) — ccpm.py:77-107.  The Sequential keeps the
    reference's slots (ZeroPad2d / Conv2d / KMaxPooling / activation per layer), so its state_dict keys are
    conv_layer.{1,5,9}.weight / .bias.  k of layer i (1-based, of L): max(3, int((1 - (i / L) ** (L - i)) * num_fields)),
    3 for the last."""

    def __init__(self, num_fields, channels=[3], kernel_heights=[3], activation="Tanh"):
        super(CCPM_ConvLayer, self).__init__()
        if not isinstance(kernel_heights, list):
            kernel_heights = [kernel_heights] * len(channels)
        elif len(kernel_heights) != len(channels):
            raise ValueError("channels={} and kernel_heights={} should have the same length."
                             .format(channels, kernel_heights))
        module_list = []
        self.num_fields = num_fields
        self.channels = [1] + channels
        self.ks = []
        self._tanh = isinstance(activation, str) and activation.lower() == "tanh"
        layers = len(kernel_heights)
        for i in range(1, len(self.channels)):
            in_channels = self.channels[i - 1]
            out_channels = self.channels[i]
            kernel_height = kernel_heights[i - 1]
            module_list.append(nn.ZeroPad2d((0, 0, kernel_height - 1, kernel_height - 1)))
            module_list.append(nn.Conv2d(in_channels, out_channels, kernel_size=(kernel_height, 1)))
            if i < layers:
                k = max(3, int((1 - pow(float(i) / layers, layers - i)) * num_fields))
            else:
                k = 3
            self.ks.append(k)
            module_list.append(KMaxPooling(k, dim=2))
            module_list.append(get_activation(activation))
        self.conv_layer = nn.Sequential(*module_list)

    def convs(self):
        return [m for m in self.conv_layer if isinstance(m, nn.Conv2d)]

    def hip_supported(self, embedding_dim: int) -> bool:
        from ... import hip
        convs = self.convs()
        return self._tanh and len(convs) > 0 and hip.ccpm_fits(
            self.num_fields, embedding_dim, [c.out_channels for c in convs], [c.kernel_size[0] for c in convs], self.ks)

    def torch_stack(self, X):
        """the reference's formulation over torch ops, wherever X lives (the pooling does not count itself here: the model
        notes the torch path once for the whole stack)"""
        for m in self.conv_layer:
            if isinstance(m, KMaxPooling):
                index = X.topk(m.k, dim=m.dim)[1].sort(dim=m.dim)[0]
                X = X.gather(m.dim, index)
            elif isinstance(m, nn.Conv2d) and X.is_cuda:
                # the (kh, 1) convolution over the already padded X as kh shifted channel products: plain GEMM-backed ops,
                # no convolution library (its per-shape search would run on the first call of every new shape)
                kh = m.kernel_size[0]
                lout = X.shape[2] - kh + 1
                X = m.bias.view(1, -1, 1, 1) + sum(torch.einsum("oc,bcld->bold", m.weight[:, :, j, 0], X[:, :, j:j + lout])
                                                   for j in range(kh))
            else:
                X = m(X)
        return X

    def forward(self, X):
        if X.is_cuda and X.dtype == torch.float32 and X.dim() == 4 and X.shape[1] == 1 and X.shape[2] == self.num_fields:
            from ... import hip
            B, D = X.shape[0], X.shape[3]
            if self.hip_supported(D):
                out = Fh.ccpm_conv_stack(X.reshape(B, self.num_fields * D), self.num_fields, D, self)
                return out.view(B, self.channels[-1], self.ks[-1], D)
            hip.note_torch_path(f"CCPM_ConvLayer over {self.num_fields} fields, D={D}, channels {self.channels[1:]} "
                                "(outside hip.ccpm_fits)")
        return self.torch_stack(X)
