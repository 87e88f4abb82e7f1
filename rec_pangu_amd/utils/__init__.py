from .evaluate import evaluate_recall, get_recall_predict

__all__ = ["evaluate_recall", "get_recall_predict"]
