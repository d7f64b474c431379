# configs/finetune_retrieval_dsl_synthetic.py with the training half of dual softmax: the model is fine-tuned with the
# dual-softmax loss (NormSoftmaxLoss(dual_softmax=T): logits (G / temperature) c softmax(T c) in both directions, the
# gradient flowing through the priors) and validated under the same prior, the best checkpoint chosen by DSL_Recall@1.
# T = 20 = 1 / temperature.  Not in the reference.
_base_ = ['finetune_retrieval_dsl_synthetic.py']
model = dict(loss_type=dict(type='NormSoftmaxLoss', cos_sim=True, temperature=0.05, dual_softmax=20.0))
evaluation = dict(interval=1, metrics=['recall_for_video_text_retrieval'], gpu_collect=True, dual_softmax=20.0,
                  save_best='DSL_Recall@1')
