"""rec_pangu_amd — MI355X-native implementation of rec_pangu's ranking forward/backward hot path.

Public surface mirrors the reference for that path only:
    rec_pangu_amd.models.ranking.{DeepFM, xDeepFM, DCN, AutoInt, FM}
    rec_pangu_amd.models.multi_task.MMOE
    rec_pangu_amd.models.sequence.{YotubeDNN, GRU4Rec, NARM, MIND, ComirecDR, SASRec, NextItNet, SRGNN, NISER, GCSAN, STAMP, ComirecSA,
        CLRec, ContraRec} (on the family's
        full-softmax loss head: DESIGN.md §18; GRU4Rec and NARM on the fused GRU recurrence: §19; MIND and ComirecDR on the fused
        capsule routing: §20; SASRec on the fused causal self-attention: §21; NextItNet on the fused dilated causal convolution
        blocks: §23; SRGNN, NISER and GCSAN on the fused session-graph gated cell: §24; STAMP and ComirecSA on the fused
        additive-attention pooling: §25; CLRec and ContraRec on the fused in-batch contrastive loss: §26)
    rec_pangu_amd.trainer.{RankTrainer, SequenceTrainer}, rec_pangu_amd.benchmark_trainer.BenchmarkTrainer
    rec_pangu_amd.dataset.{get_dataloader, SequenceDataset, SequenceDatasetV2}
    rec_pangu_amd.utils.{evaluate_recall, get_recall_predict}
Kernels: rec_pangu_amd/csrc/*.hip behind the C ABI in include/rec_pangu_hip.h, bound by rec_pangu_amd.hip.
"""
__version__ = "0.1.0"
