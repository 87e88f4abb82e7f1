"""AFM — drop-in for rec_pangu/models/ranking/afm.py:14-68.

The reference's AFM is not an attentional factorization machine: afm.py:12 carries "Fixme: change the current code of AFM
with the right version", and the class builds exactly FiBiNet's layers in the same order (LR_Layer, SENET_Layer(F, 3),
BilinearInteractionLayer(F, D, 'field_interaction'), the same MLP) and runs the same forward.  It is therefore the same
network under the reference's second name: same constructor, parameter creation order, init stream, state_dict keys and
outputs as FiBiNet, and the same kernels (see fibinet.py).
"""
from .fibinet import FiBiNet


class AFM(FiBiNet):
    def __init__(self, embedding_dim=32, hidden_units=[64, 64, 64], loss_fun='torch.nn.BCELoss()', enc_dict=None):
        super(AFM, self).__init__(embedding_dim=embedding_dim, hidden_units=hidden_units, loss_fun=loss_fun, enc_dict=enc_dict)
