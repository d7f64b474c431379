from .qa import QA_METRICS, evaluate_qa, multi_gpu_test_itm_finetune, qa_accuracy
from .retrieval import (evaluate_retrieval, multi_gpu_test_retrieval, normalize_fn,
                        recall_for_video_text_retrieval, recall_on_device)

__all__ = ['normalize_fn', 'recall_for_video_text_retrieval', 'recall_on_device', 'multi_gpu_test_retrieval', 'evaluate_retrieval',
           'multi_gpu_test_itm_finetune', 'evaluate_qa', 'qa_accuracy', 'QA_METRICS']
