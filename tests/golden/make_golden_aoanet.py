#!/usr/bin/env python
"""AOANet golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_aoanet.py

  model_aoanet_l3s4.npz   rec_pangu/models/ranking/aoanet.py:14-115 (AOANet, GeneralizedInteractionNet, GeneralizedInteraction),
                          embedding_dim=8, dnn_hidden_units=[16, 8], num_interaction_layers=3, num_subspaces=4: the default
                          stack — layer 0 over F = 5 input subspaces, two layers over 4
  model_aoanet_l1s3.npz   the same with num_interaction_layers=1, num_subspaces=3: only the P = F layer, an odd O
Both on make_golden.py's small schema and batch (seed 1234): 5 sparse + 3 dense features, the trunk's input 43 wide.  Groups
init/ batch/ out/ grad/ adam2/ adam2_out/ as make_golden.dump_model_case writes them; EVAL mode (the trunk has Dropout(0.1)).
Only data is written: no reference source, bytecode or pickled reference objects.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shim; its generators only run under __main__)

from rec_pangu.models.ranking import AOANet  # noqa: E402

CASES = {
    "aoanet_l3s4": dict(embedding_dim=8, dnn_hidden_units=[16, 8], num_interaction_layers=3, num_subspaces=4),
    "aoanet_l1s3": dict(embedding_dim=8, dnn_hidden_units=[16, 8], num_interaction_layers=1, num_subspaces=3),
}

if __name__ == "__main__":
    for name, kw in CASES.items():
        G.dump_model_case(name, lambda kw=kw: AOANet(enc_dict=G.small_enc_dict(), **kw), seed=1234, train_mode=False)
