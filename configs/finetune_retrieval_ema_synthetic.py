# Retrieval fine-tuning with the reference's `ema_hook` (tools/train.py:212-220, mmaction/core/hooks/ema.py): evaluation,
# best-checkpoint selection and every saved checkpoint use an exponential moving average of the weights (fp32, in the
# engine's slabs), training goes on with the raw ones.  total_iter is sized to the 40 iterations of this synthetic run.
_base_ = ['finetune_retrieval_synthetic.py']
ema_hook = dict(type='ExpMomentumEMAHook', momentum=0.01, total_iter=20)
