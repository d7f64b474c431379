# configs/finetune_retrieval_synthetic.py with dual-softmax re-scoring at evaluation: next to the plain Recall@K / MR keys
# the validation (tools/train.py --validate) and tools/test.py report DSL_Recall@K / DSL_MR, the ranks under
# s' = s * softmax(T * s) taken over all queries of the test set, and the best checkpoint is chosen by DSL_Recall@1.
# T = 20 = 1 / temperature of the NormSoftmaxLoss the model is trained with.  Not in the reference.
_base_ = ['finetune_retrieval_synthetic.py']
evaluation = dict(interval=1, metrics=['recall_for_video_text_retrieval'], gpu_collect=True, dual_softmax=20.0,
                  save_best='DSL_Recall@1')
