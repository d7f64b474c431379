from .qa import QA_METRICS, evaluate_qa, multi_gpu_test_itm_finetune, qa_accuracy
from .retrieval import (RETRIEVAL_METRICS, acc_for_msrvtt_mc, dual_softmax_scores, evaluate_retrieval, mc_acc_on_device,
                        multi_gpu_test_retrieval, multi_gpu_test_retrieval_varied, normalize_fn,
                        recall_for_video_text_retrieval, recall_for_video_text_retrieval_varied, recall_on_device,
                        recall_varied_on_device, sim_matrix)

__all__ = ['normalize_fn', 'recall_for_video_text_retrieval', 'recall_on_device', 'multi_gpu_test_retrieval', 'evaluate_retrieval',
           'multi_gpu_test_itm_finetune', 'evaluate_qa', 'qa_accuracy', 'QA_METRICS', 'RETRIEVAL_METRICS', 'sim_matrix',
           'acc_for_msrvtt_mc', 'recall_for_video_text_retrieval_varied', 'mc_acc_on_device', 'recall_varied_on_device',
           'multi_gpu_test_retrieval_varied', 'dual_softmax_scores']
