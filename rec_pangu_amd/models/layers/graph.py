"""The session-graph gated cell of SRGNN / NISER / GCSAN — drop-in for SRGNNConv and SRGNNCell of
rec_pangu/models/layers/graph.py (constructor signatures, parameter names, shapes and creation order as there, so state_dict
keys and the init stream match).  No dgl: the graphs of a batch are the alias list Fh.session_graph returns.

    SRGNNCell(alias int32 [B, L], hidden [B, L, D], final=False) -> one step over every sample's own graph:
        p_in = incomming_conv.lin(h), p_out = outcomming_conv.lin(h)
        in[v] = sum over transitions u -> v of p_in[u] / outdeg(u),  out[u] = sum over transitions u -> v of p_out[v] / indeg(v)
        gi = lin_ih(cat[in, out]), gh = lin_hh(h), r = s(i_r + h_r), z = s(i_i + h_i), n = tanh(i_n + r h_n)
        h' = (1 - z) h + z n
    Node v of sample b is row v of its L slots; rows behind the node count are zero on both sides of the step.  final = True
    returns the read-back of the last step in sequence order instead: (seq_hidden [B, L, D], ht [B, D]).

On the HIP device a step is one Fh.ggnn_cell node (csrc/session_graph.hip); on the CPU, and on the device
outside the kernel's limits (counted, hip.note_torch_path), Fh.ggnn_cell_reference: the same formulas as gather / scatter_add
over the padded layout.
"""
import torch
from torch import nn

from ... import functional as Fh


class SRGNNConv(nn.Module):
    """the Linear of one direction's messages; the aggregation itself belongs to the cell's step (it needs the graph)"""

    def __init__(self, dim):
        super(SRGNNConv, self).__init__()
        self.lin = torch.nn.Linear(dim, dim)

    def forward(self, hidden):
        return self.lin(hidden)


class SRGNNCell(nn.Module):
    def __init__(self, dim):
        super(SRGNNCell, self).__init__()

        self.dim = dim
        self.incomming_conv = SRGNNConv(dim)
        self.outcomming_conv = SRGNNConv(dim)

        self.lin_ih = nn.Linear(2 * dim, 3 * dim)
        self.lin_hh = nn.Linear(dim, 3 * dim)

    def forward(self, alias, hidden, final=False):
        return Fh.ggnn_cell(hidden, alias, self, final=final)

    def encode(self, alias, hidden, step):
        """`step` >= 1 steps -> the last step's (seq_hidden [B, L, D], ht [B, D])"""
        if int(step) < 1:
            raise ValueError(f"SRGNNCell.encode: step must be at least 1, got {step} (the read-back belongs to a step)")
        for _ in range(int(step) - 1):
            hidden = self(alias, hidden)
        return self(alias, hidden, final=True)
