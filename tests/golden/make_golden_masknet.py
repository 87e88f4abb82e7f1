#!/usr/bin/env python
"""MaskNet golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_masknet.py

  model_masknet_par3.npz   rec_pangu/models/ranking/masknet.py:13-87 over rec_pangu/models/layers/interaction.py:254-283
                           (MaskBlock), embedding_dim=8, block_num=3, use_parallel=True, hidden_units=[16, 8]
  model_masknet_ser2.npz   the same with block_num=2, use_parallel=False
Both on make_golden.py's small schema and batch (seed 1234): d = 5 * 8 + 3 = 43 and the mask bottleneck int(43 * 0.3) = 12
wide — every width odd.  Groups init/ batch/ out/ grad/ adam2/ adam2_out/ as make_golden.dump_model_case writes them; EVAL
mode (the MLP behind the blocks has Dropout(0.1): masknet.py:48-50).
Only data is written: no reference source, bytecode or pickled reference objects.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shim; its generators only run under __main__)

from rec_pangu.models.ranking import MaskNet  # noqa: E402

CASES = {
    "masknet_par3": dict(embedding_dim=8, block_num=3, use_parallel=True, hidden_units=[16, 8]),
    "masknet_ser2": dict(embedding_dim=8, block_num=2, use_parallel=False, hidden_units=[16, 8]),
}

if __name__ == "__main__":
    for name, kw in CASES.items():
        G.dump_model_case(name, lambda kw=kw: MaskNet(enc_dict=G.small_enc_dict(), **kw), seed=1234, train_mode=False)
