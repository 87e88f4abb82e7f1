"""Feature-interaction blocks of the hot path — drop-ins for rec_pangu/models/layers/interaction.py:
InnerProductLayer (:12-52, the two pooling outputs the ranking models use), FM_Layer (:225-235),
CrossInteractionLayer / CrossNet (:119-141), CompressedInteractionNet (:144-171), MaskBlock (:254-283), BilinearInteractionLayer
(:55-81), SENET_Layer (:238-251); GeneralizedInteractionNet / GeneralizedInteraction, which the reference keeps beside its model
(ranking/aoanet.py:81-115).
Parameter names/shapes follow the reference so its checkpoints load.
"""
from itertools import combinations

import torch
from torch import nn


class InnerProductLayer(nn.Module):
    """product_sum_pooling -> [B,1];  Bi_interaction_pooling -> [B,D]  (interaction.py:36-44).

    In DeepFM/FM on a HIP device the second-order term is produced inside the gather kernel
    (EmbeddingLayer.gather_concat(want_fm=True)), so this module is only reached with an explicit
    [B,F,D] tensor."""
    _SUPPORTED = ("product_sum_pooling", "Bi_interaction_pooling")

    def __init__(self, num_fields=None, output="product_sum_pooling"):
        super(InnerProductLayer, self).__init__()
        if output not in self._SUPPORTED:
            raise ValueError("InnerProductLayer output={} is not supported.".format(output))
        self._output_type = output

    def forward(self, feature_emb):
        if feature_emb.is_cuda and feature_emb.dtype == torch.float32 and feature_emb.shape[-1] % 4 == 0:
            from ... import functional as Fh
            return Fh.fm_pool(feature_emb, self._output_type == "Bi_interaction_pooling")
        field_sum = feature_emb.sum(dim=1)
        bi = 0.5 * (field_sum * field_sum - (feature_emb * feature_emb).sum(dim=1))
        if self._output_type == "Bi_interaction_pooling":
            return bi
        return bi.sum(dim=-1, keepdim=True)


class FM_Layer(nn.Module):
    def __init__(self, final_activation=None, use_bias=True):
        super(FM_Layer, self).__init__()
        self.inner_product_layer = InnerProductLayer(output="product_sum_pooling")
        self.final_activation = final_activation

    def forward(self, feature_emb_list):
        out = self.inner_product_layer(feature_emb_list)
        return out if self.final_activation is None else self.final_activation(out)


class CrossInteractionLayer(nn.Module):
    """one DCN-v1 cross layer: (X_i . w) * X_0 + b   (interaction.py:119-127)"""

    def __init__(self, input_dim):
        super(CrossInteractionLayer, self).__init__()
        self.weight = nn.Linear(input_dim, 1, bias=False)
        self.bias = nn.Parameter(torch.zeros(input_dim))

    def forward(self, X_0, X_i):
        return self.weight(X_i) * X_0 + self.bias


class CrossNet(nn.Module):
    """X_{l+1} = X_l + (X_l . w_l) X_0 + b_l   (interaction.py:130-141)"""

    def __init__(self, input_dim, num_layers):
        super(CrossNet, self).__init__()
        self.num_layers = num_layers
        self.input_dim = input_dim
        self.cross_net = nn.ModuleList(CrossInteractionLayer(input_dim) for _ in range(num_layers))

    def stacked(self):
        """([L,d] weights, [L,d] biases): the per-layer parameters stacked for the one-pass HIP kernel
        (torch.stack keeps them on the autograd tape, so the gradients flow back to each layer)."""
        W = torch.stack([layer.weight.weight.reshape(-1) for layer in self.cross_net])
        Bv = torch.stack([layer.bias for layer in self.cross_net])
        return W, Bv

    def forward(self, X_0, fc: nn.Linear = None):
        """X_L [B,d]; with `fc` (a Linear(d,1), as in DCN) the fused kernel returns fc(X_L) [B,1] instead."""
        if X_0.is_cuda:
            from ... import functional as Fh
            lw = [layer.weight.weight for layer in self.cross_net]
            lb = [layer.bias for layer in self.cross_net]
            if fc is not None:
                return Fh.crossnet(X_0, lw, lb, fc.weight, fc.bias)
            return Fh.crossnet(X_0, lw, lb)
        X_i = X_0
        for layer in self.cross_net:
            X_i = X_i + layer(X_0, X_i)
        return X_i if fc is None else fc(X_i)


class CompressedInteractionNet(nn.Module):
    """CIN (interaction.py:144-171): X_k[b,o,:] = sum_{h,m} W_k[o, h*M+m] X_0[b,h,:] X_{k-1}[b,m,:] + bias_k[o];
    no activation, no split-half; sum-pool over the embedding axis, concat, fc -> [B, output_dim].
    Weights are kept as Conv1d(kernel_size=1) modules for state_dict compatibility
    (`cin_layer.layer_k.weight` is [O, H*M, 1])."""

    def __init__(self, num_fields, cin_layer_units, output_dim=1):
        super(CompressedInteractionNet, self).__init__()
        self.cin_layer_units = cin_layer_units
        self.num_fields = num_fields
        self.fc = nn.Linear(sum(cin_layer_units), output_dim)
        self.cin_layer = nn.ModuleDict()
        prev = num_fields
        for i, unit in enumerate(cin_layer_units):
            self.cin_layer["layer_" + str(i + 1)] = nn.Conv1d(num_fields * prev, unit, kernel_size=1)
            prev = unit

    def _forward_hip(self, feature_emb, as_list: bool = False):
        """Every layer but the last runs at full width and keeps X_k for the next one, in the kernel form functional.cin_forms
        chose for it.  The LAST layer only feeds sum-pooling and `fc`, both linear, and the CIN has no activation, so
            sum_o c[o] * sum_d X_L[b,o,d] = sum_d sum_{h,m} V[h,m] X_0[b,h,d] X_{L-1}[b,m,d] + D * (c . bias_L),
            V = sum_o c[o] W_L[o]            (c = the slice of fc.weight that multiplies the last layer's pooling)
        and it is evaluated as a single-output-channel layer with weights V: 1/O_L of the work, same algebra."""
        from ... import functional as Fh
        if feature_emb.dim() == 2:  # (already the [B, H D] row buffer: a model that hands over its own view of x)
            B, H, x0 = feature_emb.shape[0], self.num_fields, feature_emb
            D = x0.shape[1] // H
        else:
            B, H, D = feature_emb.shape
            x0 = feature_emb.reshape(B, H * D)
        plan = Fh.cin_forms(H, self.cin_layer_units, D, None, x0.stride(0) % 4 == 0 and x0.data_ptr() % 16 == 0,
                            self.fc.weight.shape[0])
        if plan is None:
            raise NotImplementedError("no HIP form of this CIN (functional.cin_forms): forward() composes it from device ops")
        if plan.x0_contiguous:
            x0 = x0.contiguous()
        L, last = len(plan.layers), plan.layers[-1]
        # form "head": with a layer in front of the last one the whole head is library launches — fc.weight split without autograd
        # slice nodes, V = c . W_L / c . b_L / the scalars / their gradients in cin_head, the last layer's gradient of X_0 added
        # into the first layer's inside its backward (CINLink)
        link = Fh.CINLink() if (last.fwd == "head" and torch.is_grad_enabled() and x0.requires_grad) else None
        xp, M, pooled, n_prev = None, H, [], 0
        for i, form in enumerate(plan.layers[:-1]):
            conv = self.cin_layer["layer_" + str(i + 1)]
            O = conv.weight.shape[0]
            X_i, p_i = Fh.cin_layer(x0, xp, conv.weight.view(O, H * M), conv.bias, H, M, D, form, link=link if i == 0 else None)
            pooled.append(p_i)
            xp, M, n_prev = X_i.view(B, O * D), O, n_prev + O
        conv = self.cin_layer["layer_" + str(L)]
        O = conv.weight.shape[0]
        if last.fwd == "head":
            c_prev, c_last = Fh.row_split(self.fc.weight, n_prev)
            head = Fh.cin_head(x0, xp, conv.weight.view(O, H * M), conv.bias, c_last, self.fc.bias, H, M, D, link)
            pool_logit = Fh.linear_act(pooled[0] if len(pooled) == 1 else torch.cat(pooled, dim=-1), c_prev, None)
            return [head, pool_logit] if as_list else head + pool_logit
        c_last = self.fc.weight[:, n_prev:]                                  # [out_dim, O_L]
        V = c_last @ conv.weight.view(O, H * M)                              # [1, H*M]   (weight-space, tiny)
        vb = (c_last @ conv.bias.view(O, 1)).view(1)                         # c . bias_L
        if last.fwd == "last":
            # dedicated HBM-bound kernels for the single collapsed channel; the bias enters as D * (c . bias_L)
            logit = Fh.cin_last(x0, V, H, D) + D * vb
        else:
            logit = Fh.cin_layer(x0, xp, V, vb, H, M, D, last, want_out=False)  # [B,1] = sum_o c[o] pooled_L[b,o]
        if pooled:
            logit = logit + Fh.linear_act(torch.cat(pooled, dim=-1), self.fc.weight[:, :n_prev].contiguous(), None)
        logit = logit + self.fc.bias
        return [logit] if as_list else logit

    def hip_supported(self, H, D=None) -> bool:
        """does a kernel form exist for every layer (functional.cin_forms has the table)?  Otherwise forward() composes the
        CIN from device ops."""
        from ... import functional as Fh
        return Fh.cin_forms(H, self.cin_layer_units, D or 0, None, True, self.fc.weight.shape[0]) is not None

    def forward(self, feature_emb, as_list: bool = False):
        """as_list (HIP callers that add their logits inside the loss launch): the logit as a list of [B, 1] addends"""
        if feature_emb.dim() == 2:
            H, D = self.num_fields, feature_emb.shape[1] // self.num_fields
            if not (feature_emb.is_cuda and self.hip_supported(H, D)):
                feature_emb = feature_emb.reshape(feature_emb.shape[0], H, D)
        B = feature_emb.shape[0]
        if feature_emb.dim() == 3:
            _, H, D = feature_emb.shape
        if feature_emb.is_cuda and self.hip_supported(H, D):
            return self._forward_hip(feature_emb, as_list)
        if feature_emb.is_cuda:
            from ... import hip
            hip.note_torch_path(f"CompressedInteractionNet with {H} fields, D={D}, layers {list(self.cin_layer_units)}, "
                                f"{self.fc.weight.shape[0]} outputs (no kernel form: functional.cin_forms)")
        X_0, X_i, pooled = feature_emb, feature_emb, []
        for i in range(len(self.cin_layer_units)):
            conv = self.cin_layer["layer_" + str(i + 1)]
            M = X_i.shape[1]
            W = conv.weight.view(conv.weight.shape[0], H, M)
            # contract (h, m) without materialising the [B, H*M, D] outer product the reference builds
            t = torch.einsum("ohm,bmd->bohd", W, X_i)
            X_i = (t * X_0.unsqueeze(1)).sum(dim=2) + conv.bias.view(1, -1, 1)
            pooled.append(X_i.sum(dim=-1))
        out = self.fc(torch.cat(pooled, dim=-1))
        return [out] if as_list else out


class MaskBlock(nn.Module):
    """LN_out(hidden(LN_in(net) * mask(mask_input)))  (interaction.py:254-283): the instance-guided mask is a two-layer
    bottleneck (mask_input_dim -> int(mask_input_dim * reduction_factor) -> input_dim, ReLU between) that multiplies the
    normalised input elementwise.  Module names are the reference's (`_input_layer_norm`, `_mask_layer.{0,2}`,
    `_hidden_layer`, `_layer_norm`).

    On a HIP device: the mask's Linears and the hidden Linear are matrix-core launches, each LayerNorm one launch
    (rp_layernorm_fwd; the first one multiplies by the mask inside, so LN_in(net) is never stored).  MaskNet does not call
    its blocks one by one: it runs the whole stack on one autograd node (functional.mask_block_stack)."""

    def __init__(self, input_dim: int, mask_input_dim: int, output_size: int, reduction_factor: float) -> None:
        super(MaskBlock, self).__init__()
        self._input_layer_norm = nn.LayerNorm(input_dim)
        aggregation_size = int(mask_input_dim * reduction_factor)
        self._mask_layer = nn.Sequential(nn.Linear(mask_input_dim, aggregation_size), nn.ReLU(),
                                         nn.Linear(aggregation_size, input_dim))
        self._hidden_layer = nn.Linear(input_dim, output_size)
        self._layer_norm = nn.LayerNorm(output_size)

    def forward(self, net, mask_input):
        if net.is_cuda and net.dtype == torch.float32:
            from ... import functional as Fh
            lead = net.shape[:-1]
            net, mask_input = net.reshape(-1, net.shape[-1]), mask_input.reshape(-1, mask_input.shape[-1])
            h = Fh.linear_act(mask_input, self._mask_layer[0].weight, self._mask_layer[0].bias, Fh.ACT_RELU)
            mask = Fh.linear_act(h, self._mask_layer[2].weight, self._mask_layer[2].bias)
            hidden = Fh.linear_act(Fh.layer_norm(net, self._input_layer_norm, mul=mask), self._hidden_layer.weight,
                                   self._hidden_layer.bias)
            return Fh.layer_norm(hidden, self._layer_norm).reshape(*lead, -1)
        masked = self._input_layer_norm(net) * self._mask_layer(mask_input)
        return self._layer_norm(self._hidden_layer(masked))


class GeneralizedInteraction(nn.Module):
    """One layer of AOANet's generalized interaction net (ranking/aoanet.py:97-115): B_0 [B, F, D] against B_i [B, P, D]
    (P = input_subspaces) -> [B, O, D].  The reference builds the outer product of every (subspace, field) pair —
    [B, P F, D, D] — and then contracts it with alpha, W and h; the same result factorises, with M[o,h,d] = W[o,h,d] h[o,d]:
        T[b,o,p,h] = sum_d M[o,h,d] B_i[b,p,d]    U[b,o,p,h] = sum_f alpha[p F + f, o] B_0[b,f,h]    out[b,o,h] = sum_p T U
    (the alpha row is p F + f: the reference's repeat / view pair).  forward() computes that form; on a HIP device the whole
    net runs as functional.gin_stack (rp_gin_fwd / rp_gin_bwd), this module alone composes it from device ops (counted)."""

    def __init__(self, input_subspaces, output_subspaces, num_fields, embedding_dim):
        super(GeneralizedInteraction, self).__init__()
        self.input_subspaces = input_subspaces
        self.num_fields = num_fields
        self.embedding_dim = embedding_dim
        self.W = nn.Parameter(torch.eye(embedding_dim, embedding_dim).unsqueeze(0).repeat(output_subspaces, 1, 1))
        self.alpha = nn.Parameter(torch.ones(input_subspaces * num_fields, output_subspaces))
        self.h = nn.Parameter(torch.ones(output_subspaces, embedding_dim, 1))

    def factorised(self, B_0, B_i):
        M = self.W * self.h.squeeze(-1).unsqueeze(1)
        T = torch.einsum("ohd,bpd->boph", M, B_i)
        U = torch.einsum("pfo,bfh->boph", self.alpha.view(self.input_subspaces, self.num_fields, -1), B_0)
        return (T * U).sum(dim=2)

    def forward(self, B_0, B_i):
        if B_0.is_cuda:
            from ... import hip
            hip.note_torch_path("GeneralizedInteraction called on its own (the kernels run the whole net: "
                                "GeneralizedInteractionNet / functional.gin_stack)")
        return self.factorised(B_0, B_i)


class GeneralizedInteractionNet(nn.Module):
    """B_{i+1} = layer_i(B_0, B_i), B_0 = the field embeddings (ranking/aoanet.py:81-94); layer 0 has F input subspaces, the
    others num_subspaces.  On a HIP device the stack is one autograd node, one launch per layer each way
    (functional.gin_stack).  B_0 is [B, F, D] and the result [B, O, D], as in the reference."""

    def __init__(self, num_layers, num_subspaces, num_fields, embedding_dim):
        super(GeneralizedInteractionNet, self).__init__()
        self.num_fields, self.embedding_dim = num_fields, embedding_dim
        self.layers = nn.ModuleList([GeneralizedInteraction(num_fields if i == 0 else num_subspaces, num_subspaces,
                                                            num_fields, embedding_dim) for i in range(num_layers)])

    def hip_supported(self) -> bool:
        from ... import hip
        return len(self.layers) > 0 and all(hip.gin_fits(l.num_fields, l.input_subspaces, l.W.shape[0], l.embedding_dim)
                                            for l in self.layers)

    def forward(self, B_0):
        F, D = self.num_fields, self.embedding_dim
        if B_0.is_cuda and B_0.dtype == torch.float32 and len(self.layers) > 0:
            from ... import functional as Fh, hip
            if self.hip_supported():
                return Fh.gin_stack(B_0.reshape(B_0.shape[0], F * D), F, D, self.layers).view(B_0.shape[0], -1, D)
            hip.note_torch_path(f"GeneralizedInteractionNet over {F} fields, D={D}, {self.layers[0].W.shape[0]} subspaces "
                                "(outside hip.gin_fits)")
        B_i = B_0
        for layer in self.layers:
            B_i = layer.factorised(B_0, B_i)
        return B_i


class BilinearInteractionLayer(nn.Module):
    """T[b, p, :] = (W_w(p) E[b, i, :]) * E[b, j, :] for the field pairs p = (i, j), i < j, in itertools.combinations order ->
    [B, P, D]  (interaction.py:55-81).  "field_all": one matrix (`bilinear_layer.weight`); "field_each": matrix i for the pairs
    (i, .) — num_fields modules, the last one unused, as upstream; "field_interaction": one per pair
    (`bilinear_layer.{p}.weight`).  On a HIP device the layer is one launch each way (functional.senet_bilinear without a
    SENET: rp_bilinear_fwd with R = 0); FiBiNet runs it fused with its SENET_Layer instead of calling it twice."""

    def __init__(self, num_fields, embedding_dim, bilinear_type="field_interaction"):
        super(BilinearInteractionLayer, self).__init__()
        self.bilinear_type = bilinear_type
        if self.bilinear_type == "field_all":
            self.bilinear_layer = nn.Linear(embedding_dim, embedding_dim, bias=False)
        elif self.bilinear_type == "field_each":
            self.bilinear_layer = nn.ModuleList([nn.Linear(embedding_dim, embedding_dim, bias=False)
                                                 for i in range(num_fields)])
        elif self.bilinear_type == "field_interaction":
            self.bilinear_layer = nn.ModuleList([nn.Linear(embedding_dim, embedding_dim, bias=False)
                                                 for i, j in combinations(range(num_fields), 2)])
        else:
            raise NotImplementedError()

    def weights(self):
        """the [D, D] matrices in the order the kernels number them"""
        if self.bilinear_type == "field_all":
            return [self.bilinear_layer.weight]
        return [m.weight for m in self.bilinear_layer]

    def torch_pairs(self, feature_emb):
        """the reference's formulation over torch ops, wherever feature_emb lives"""
        feature_emb_list = torch.split(feature_emb, 1, dim=1)
        if self.bilinear_type == "field_all":
            bilinear_list = [self.bilinear_layer(v_i) * v_j for v_i, v_j in combinations(feature_emb_list, 2)]
        elif self.bilinear_type == "field_each":
            bilinear_list = [self.bilinear_layer[i](feature_emb_list[i]) * feature_emb_list[j]
                             for i, j in combinations(range(len(feature_emb_list)), 2)]
        else:
            bilinear_list = [self.bilinear_layer[i](v[0]) * v[1] for i, v in enumerate(combinations(feature_emb_list, 2))]
        return torch.cat(bilinear_list, dim=1)

    def forward(self, feature_emb):
        if feature_emb.is_cuda and feature_emb.dtype == torch.float32 and feature_emb.dim() == 3:
            from ... import functional as Fh, hip
            B, F, D = feature_emb.shape
            if hip.bilinear_fits(F, D, 0, self.bilinear_type) and len(self.weights()) == hip.bilinear_weight_count(
                    F, self.bilinear_type):
                return Fh.senet_bilinear(feature_emb.reshape(B, F * D), F, D, None, self, pad_to=1).view(B, -1, D)
            hip.note_torch_path(f"BilinearInteractionLayer over {F} fields, D={D}, {self.bilinear_type} (outside hip.bilinear_fits)")
        return self.torch_pairs(feature_emb)


class SENET_Layer(nn.Module):
    """V = E * A[..., None] with A = relu(W2 relu(W1 mean_d E)), no biases, reduced size max(1, int(F / ratio))
    (interaction.py:238-251; `excitation.{0,2}.weight`).  FiBiNet on a HIP device never forms V: A_i A_j scales the bilinear
    products inside rp_bilinear_fwd (functional.senet_bilinear).  Called on its own with a HIP tensor the layer composes V from
    device ops (counted: hip.note_torch_path)."""

    def __init__(self, num_fields, reduction_ratio=3):
        super(SENET_Layer, self).__init__()
        reduced_size = max(1, int(num_fields / reduction_ratio))
        self.excitation = nn.Sequential(nn.Linear(num_fields, reduced_size, bias=False),
                                        nn.ReLU(),
                                        nn.Linear(reduced_size, num_fields, bias=False),
                                        nn.ReLU())

    def weights_A(self, feature_emb):
        return self.excitation(torch.mean(feature_emb, dim=-1))

    def forward(self, feature_emb):
        if feature_emb.is_cuda:
            from ... import hip
            hip.note_torch_path("SENET_Layer called on its own (the kernels run it inside the bilinear interaction: "
                                "functional.senet_bilinear)")
        return feature_emb * self.weights_A(feature_emb).unsqueeze(-1)
