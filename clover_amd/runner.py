"""Runner + config layer under a tools/train.py-style driver, restated from the reference:

* ``Config``: python config files with ``_base_`` inheritance, attribute access and ``--cfg-options a.b=c``
  overrides (what ``mmcv.Config.fromfile`` / ``merge_from_dict`` give ``tools/train.py:261-263``; mmcv is not
  installed here);
* ``scaled_lr``: the linear scaling rule of ``tools/train.py:160-166``;
* ``CloverRunner``: epoch loop, hook call points and the multi-dataloader interleave of
  ``mmaction/core/runner/clover_runner.py:17-35,60-96`` (one optimizer step per loader per batch index), including
  its behaviour once the shorter loader is exhausted;
* checkpoints in the reference's ``{'meta', 'state_dict', 'optimizer'}`` layout (``epoch_based_runner.py:25-58``);
* ``EvalHook``: validation during training — schedule, rule inference and best-checkpoint keeping of
  ``mmaction/core/hooks/my_eval_hook.py:404-880`` (``tools/train.py --validate``, ``tools/train.py:192-209``);
* ``ExpMomentumEMAHook`` / ``LinearMomentumEMAHook``: the ``ema_hook`` of ``tools/train.py:212-220``
  (``mmaction/core/hooks/ema.py``) — schedules and call points here, the average itself in ``CloverEngine``.

The step itself is ``CloverEngine.step`` (or any object with ``train_step``); nothing here touches the GPU except the
test loops ``EvalHook`` calls (``clover_amd.evaluation``).
"""
import ast
import copy
import math
import os
import runpy
import time
from itertools import zip_longest

import torch


# --------------------------------------------------------------------------- config
class ConfigDict(dict):
    """dict with attribute access (nested dicts are wrapped on read)."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError as e:
            raise AttributeError(k) from e
        if isinstance(v, dict) and not isinstance(v, ConfigDict):
            v = ConfigDict(v)
            self[k] = v                                  # wrap in place: mutations through the view must stick
        return v

    def __setattr__(self, k, v):
        self[k] = v


def _merge(base, child):
    """mmcv semantics: dicts merge recursively, anything else is replaced; ``_delete_=True`` in the child dict
    drops the base dict instead of merging into it."""
    out = copy.deepcopy(base)
    for k, v in child.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get('_delete_', False):
            out[k] = _merge(out[k], v)
        else:
            out[k] = copy.deepcopy({kk: vv for kk, vv in v.items() if kk != '_delete_'} if isinstance(v, dict) else v)
    return out


class Config:
    def __init__(self, cfg_dict=None, filename=None):
        object.__setattr__(self, '_cfg', ConfigDict(cfg_dict or {}))
        object.__setattr__(self, 'filename', filename)

    @staticmethod
    def _load(path):
        ns = runpy.run_path(path)
        cfg = {k: v for k, v in ns.items() if not k.startswith('__') and not callable(v)
               and not isinstance(v, type(os))}
        bases = cfg.pop('_base_', [])
        bases = [bases] if isinstance(bases, str) else list(bases)
        merged = {}
        for b in bases:
            merged = _merge(merged, Config._load(os.path.join(os.path.dirname(path), b)))
        return _merge(merged, cfg)

    @classmethod
    def fromfile(cls, path):
        return cls(cls._load(os.path.abspath(path)), filename=path)

    def merge_from_dict(self, options):
        """``{'model.backbone.depths': [2, 2]}`` style overrides (tools/train.py:263)."""
        for key, val in (options or {}).items():
            d = self._cfg
            parts = key.split('.')
            for p in parts[:-1]:
                d = d.setdefault(p, {})
            d[parts[-1]] = val

    def __getattr__(self, k):
        return getattr(self._cfg, k)

    def __setattr__(self, k, v):
        self._cfg[k] = v

    def get(self, k, default=None):
        return self._cfg.get(k, default)

    def setdefault(self, k, v):
        return self._cfg.setdefault(k, v)

    def to_dict(self):
        return copy.deepcopy(dict(self._cfg))


def parse_cfg_options(items):
    """['a.b=1', 'c=[1,2]', 'd=text'] -> dict (mmcv DictAction)."""
    out = {}
    for it in items or []:
        k, v = it.split('=', 1)
        try:
            out[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            out[k] = v
    return out


def scaled_lr(cfg, world_size):
    """tools/train.py:160-166 — if the optimizer config carries ``base_lr`` it is REMOVED and
    ``lr = base_lr * videos_per_gpu * world_size`` is set, with videos_per_gpu read from the TOP level of the
    config (``cfg.get('videos_per_gpu', 1)``, not ``cfg.data``), exactly as the reference does.  The rule is base_lr times
    the GLOBAL batch: ``virtual_ranks = k`` (top level) counts as k more ranks."""
    opt = cfg.optimizer
    if 'base_lr' in opt:
        base_lr = opt.pop('base_lr')
        opt['lr'] = base_lr * cfg.get('videos_per_gpu', 1) * world_size * int(cfg.get('virtual_ranks', 1) or 1)
    return opt.get('lr')


class GroupedLoader:
    """Lists of k consecutive batches of ``loader`` — the k micro-batches of one virtual-rank step
    (``CloverEngine(virtual_ranks=k).step``), in the loader's order: micro-batch j of step i is batch ``i * k + j``.
    ``len`` is ``len(loader) // k``; a remainder is dropped, said once in one printed line."""

    def __init__(self, loader, k, printer=print):
        if int(k) < 1:
            raise ValueError(f'GroupedLoader: k must be >= 1, got {k}')
        self.loader, self.k = loader, int(k)
        rest = len(loader) % self.k
        if rest and printer is not None:
            printer(f'virtual_ranks={self.k}: the last {rest} of {len(loader)} batches per epoch do not fill a step and '
                    'are dropped')

    def __len__(self):
        return len(self.loader) // self.k

    def __iter__(self):
        group = []
        for batch in self.loader:
            group.append(batch)
            if len(group) == self.k:
                yield group
                group = []


# --------------------------------------------------------------------------- runner
class Hook:
    """The six call points the reference's runners use (mmcv Hook names)."""

    def before_run(self, runner): pass
    def after_run(self, runner): pass
    def before_train_epoch(self, runner): pass
    def after_train_epoch(self, runner): pass
    def before_train_iter(self, runner): pass
    def after_train_iter(self, runner): pass


class LrUpdaterHook(Hook):
    """mmcv 1.3.x ``CosineAnnealingLrUpdaterHook`` with ``by_epoch=False`` and linear warm-up (the reference's
    ``lr_config``, pretrain_webvid_cc3m.py:139-140).  The schedule is indexed by ``runner.iter`` —
    which the multi-loader runner advances once per batch INDEX, so both loaders' steps of one index share one LR
    (clover_runner.py:76-91) — against ``runner._max_iters`` (epochs x the LONGEST loader), and ``warmup_iters`` given
    in epochs is multiplied by that loader's length in ``before_train_epoch`` as mmcv does.  ``before_train_iter``
    hands the value to the stepper (``set_lr``), i.e. before the step that uses it, starting at iter 0."""

    def __init__(self, base_lr, min_lr_ratio=None, min_lr=None, warmup=None, warmup_iters=0, warmup_ratio=0.1,
                 warmup_by_epoch=False, **_ignored):
        assert (min_lr is None) ^ (min_lr_ratio is None), 'exactly one of min_lr / min_lr_ratio'
        assert warmup in (None, 'linear'), 'only linear warm-up is restated'
        self.base_lr = base_lr
        self.min_lr_ratio = min_lr_ratio if min_lr_ratio is not None else min_lr / base_lr
        self.warmup, self.warmup_ratio = warmup, warmup_ratio
        self.warmup_epochs = warmup_iters if warmup_by_epoch else None
        self.warmup_iters = None if warmup_by_epoch else warmup_iters
        self.history = []

    def before_train_epoch(self, runner):
        if self.warmup_iters is None:
            self.warmup_iters = self.warmup_epochs * runner.epoch_len

    def lr_at(self, it, max_iters):
        from .engine import cosine_lr
        return cosine_lr(self.base_lr, it, max_iters, self.min_lr_ratio,
                         self.warmup_iters if self.warmup else 0, self.warmup_ratio)

    def before_train_iter(self, runner):
        lr = self.lr_at(runner.iter, runner._max_iters)
        self.history.append(lr)
        if hasattr(runner.stepper, 'set_lr'):
            runner.stepper.set_lr(lr)


class LogHook(Hook):
    """TextLoggerHook stand-in: keeps the last ``log_vars`` (same keys the reference logs) every `interval` iters."""

    def __init__(self, interval=10, printer=None):
        self.interval, self.printer, self.records = interval, printer, []

    def after_train_iter(self, runner):
        if runner.inner_iter % self.interval == 0 and runner.outputs is not None:
            rec = dict(epoch=runner.epoch + 1, iter=runner.inner_iter + 1,
                       **{k: float(v) for k, v in dict(runner.outputs['log_vars']).items()})
            self.records.append(rec)
            if self.printer:
                self.printer(rec)


class OverflowHook(Hook):
    """What mmcv prints on every fp16 log line and what ``Fp16OptimizerHook`` warns about (mmcv_Fp16OptimizerHook.py:123-141),
    for an engine whose loss scaler, overflow test and skip decision never leave the device.

    Every ``interval`` optimizer steps ONE read of the engine's optimizer record (``engine.step_stats()``, a host sync)
    gives a record ``dict(epoch, iter, loss_scale, grad_norm, skipped)`` (``records``).  If ``skipped`` grew since the last
    look, the engine's overflow report (``engine.overflow_report()``: needs ``CloverEngine(overflow_report=True)``) is
    printed: the ``top`` parameters by count of non-finite gradient elements, then by largest finite magnitude.  With
    ``max_consecutive_skips = N`` a run of N skipped steps in a row raises ``RuntimeError`` with the scale and those
    parameters — a static scale that overflows skips every step from then on, and says nothing.  When the engine also
    scans its forward outputs (``CloverEngine(activation_report=True)``: the report has ``activations``) the text gains a
    forward line — the first watched module whose output was non-finite, or that all were finite — and the error names
    that module: a forward overflow makes EVERY gradient non-finite, and no loss scale cures it.  The run is derived from the
    ``skipped`` and ``calls`` deltas between two looks: every step of the window skipped extends it, none skipped ends it;
    a window with both (possible with ``interval > 1`` only) restarts it from what is known, the last step."""

    def __init__(self, interval=10, top=5, max_consecutive_skips=None, printer=None):
        assert interval >= 1 and top >= 1 and (max_consecutive_skips is None or max_consecutive_skips >= 1)
        self.interval, self.top, self.max_consecutive_skips = interval, top, max_consecutive_skips
        self.printer = print if printer is None else printer
        self.records, self.run_of_skips = [], 0
        self._steps, self._last = 0, None

    def before_run(self, runner):
        eng = runner.stepper
        missing = [a for a in ('step_stats', 'overflow_report') if not hasattr(eng, a)]
        if missing:
            raise TypeError(f'{type(self).__name__}: the skip decision lives in the CloverEngine; the stepper '
                            f'{type(eng).__name__} has no {", ".join(missing)} — drive the run with a CloverEngine')
        self._last = eng.step_stats()

    @staticmethod
    def top_rows(report, top):
        return sorted(report['rows'], key=lambda r: (-r[2], -r[3]))[:top]

    def describe(self, report):
        rows = self.top_rows(report, self.top)
        lines = [f'overflow: step skipped ({report["skipped"]} so far, {report["t"]} taken) at loss_scale '
                 f'{report["loss_scale"]:g}; {len(report["rows"])} parameter(s) with non-finite gradients, top {len(rows)}:']
        lines += [f'  {name}: {nf} of {numel} non-finite, max |g| {mx:.4g}, norm {norm:.4g} over the finite ones'
                  for name, numel, nf, mx, norm in rows]
        if 'activations' in report:            # an engine with activation_report=True: where the FORWARD pass broke, if it did
            lines.append(self.describe_forward(report['activations']))
        return '\n'.join(lines)

    @staticmethod
    def describe_forward(activations):
        rows = activations['rows']
        if activations['first'] is None:
            return 'forward outputs all finite: the overflow arose in the backward pass or the loss'
        name, numel, calls, nf, _ = rows[0]
        return (f'forward: first non-finite output at {name} ({nf} of {numel * calls}), {len(rows) - 1} watched modules '
                'downstream')

    def after_train_iter(self, runner):
        self._steps += 1
        if self._steps % self.interval != 0:
            return
        eng = runner.stepper
        st, last = eng.step_stats(), self._last
        self._last = st
        self.records.append(dict(epoch=runner.epoch + 1, iter=runner.inner_iter + 1, loss_scale=st['loss_scale'],
                                 grad_norm=st['grad_norm'], skipped=st['skipped']))
        d_skipped, d_calls = st['skipped'] - last['skipped'], st['calls'] - last['calls']
        if d_skipped <= 0:
            self.run_of_skips = 0
            return
        self.run_of_skips = self.run_of_skips + d_skipped if d_skipped == d_calls else int(bool(st.get('skip', 0)))
        report = eng.overflow_report()
        if report is not None:
            self.printer(self.describe(report))
        if self.max_consecutive_skips is not None and self.run_of_skips >= self.max_consecutive_skips:
            names = ', '.join(r[0] for r in self.top_rows(report, self.top)) if report else 'no report'
            first = ((report or {}).get('activations') or {}).get('first')
            raise RuntimeError(f'{self.run_of_skips} optimizer steps in a row were skipped for non-finite gradients at '
                               f'loss_scale {st["loss_scale"]:g} (max_consecutive_skips={self.max_consecutive_skips}); '
                               f'parameters with non-finite gradients: {names}' + (
                                   f'; first non-finite forward output: {first}' if first else ''))


class CheckpointHook(Hook):
    def __init__(self, out_dir, interval=1):
        self.out_dir, self.interval = out_dir, interval

    def after_train_epoch(self, runner):
        if (runner.epoch + 1) % self.interval == 0:
            runner.save_checkpoint(self.out_dir, f'epoch_{runner.epoch + 1}.pth')



class EvalHook(Hook):
    """``MyEvalHook`` + ``MyDistEvalHook`` (my_eval_hook.py:404-880): every ``interval`` epochs (or iterations with
    ``by_epoch=False``) run the test loop over ``dataloader``, compute the metrics, log them and keep the best checkpoint.

    ``test_fn``: ``'recall_for_video_text_retrieval'`` or None -> ``multi_gpu_test_retrieval`` + ``evaluate_retrieval``
    (embeddings stay on the device, ranks from ``ops.retrieval_rank``; with ``'video_qa_mc'`` among ``metrics`` the loop
    also collects the labels — zero-shot multiple choice, ``ops.retrieval_group_best`` —, with
    ``'recall_for_video_text_retrieval_varied'`` it is ``multi_gpu_test_retrieval_varied``); ``'use_itm_head_fn'`` ->
    ``multi_gpu_test_itm_finetune`` + ``evaluate_qa``; a callable ``test_fn(model, dataloader)`` returns the metrics dict
    itself.  ``dual_softmax = T`` (``evaluation = dict(..., dual_softmax=T)``) adds the ``DSL_*`` keys of the two recall
    metrics — ranks under the dual-softmax prior, ``ops.retrieval_rank(..., dual_softmax=T)`` — next to the plain ones
    (``save_best='DSL_Recall@1'`` follows the ``Recall@`` rule); multiple choice and video QA refuse it.
    EVERY rank runs the test loop (its collection is a collective); rank 0 alone evaluates, appends
    ``dict(epoch, **metrics)`` to ``records``, prints it through ``printer`` (what ``LogHook`` is given) and saves.
    The best score and path live in ``runner.meta['hook_msgs']`` (``best_score``, ``best_ckpt``), which checkpoints carry
    and ``CloverRunner.resume`` restores; the best checkpoint is ``{basename(work_dir)}_best_{key}_epoch_{n}.pth`` and
    replaces the previous best file (:693-707).

    The test loop runs eagerly between the engine's graph replays, in ``model.eval()`` under ``no_grad``.  An engine-bound
    model computes from the 16-bit shadows AdamW rewrites in place (``param._clv_shadow``, read per call by ``ops``), so it
    sees the current weights; the loop feeds its own batches, never the graphs' static inputs, draws no dropout seed
    (p = 0 in eval mode) and runs no backward, so the first-touch state stays as the last step left it.  ``_guard`` checks
    those three, and the model's mode, around every evaluation."""

    rule_map = {'greater': lambda x, y: x > y, 'less': lambda x, y: x < y}
    init_value_map = {'greater': -float('inf'), 'less': float('inf')}
    _default_greater_keys = ['acc', 'top', 'AR@', 'auc', 'precision', 'mAP', 'mDice', 'mIoU', 'mAcc', 'aAcc', 'Recall@',
                             'accuracy']
    _default_less_keys = ['loss']

    def __init__(self, dataloader, start=None, interval=1, by_epoch=True, save_best='auto', rule=None, test_fn=None,
                 greater_keys=None, less_keys=None, gpu_collect=True, metrics=None, broadcast_bn_buffer=True,
                 printer=None, dual_softmax=None):
        if interval <= 0:
            raise ValueError(f'interval must be a positive number, but got {interval}')
        assert isinstance(by_epoch, bool), '``by_epoch`` should be a boolean'
        if start is not None and start < 0:
            raise ValueError(f'The evaluation start epoch {start} is smaller than 0')
        assert isinstance(save_best, str) or save_best is None, f'"save_best" should be a str or None, not {type(save_best)}'
        self.dataloader, self.interval, self.start, self.by_epoch = dataloader, interval, start, by_epoch
        self.save_best, self.initial_flag = save_best, True
        if test_fn is not None and not callable(test_fn) and test_fn not in ('recall_for_video_text_retrieval',
                                                                              'use_itm_head_fn'):
            raise KeyError(f'test_fn {test_fn!r}: recall_for_video_text_retrieval, use_itm_head_fn or a callable')
        self.test_fn = test_fn
        if metrics is None:
            metrics = ['video_qa_mc'] if test_fn == 'use_itm_head_fn' else ['recall_for_video_text_retrieval']
        self.metrics = [metrics] if isinstance(metrics, str) else list(metrics)
        self.dual_softmax = None if dual_softmax is None else float(dual_softmax)
        if self.dual_softmax is not None and (callable(test_fn) or test_fn == 'use_itm_head_fn' or
                                              'video_qa_mc' in self.metrics):
            from .evaluation.retrieval import _NO_DSL_MC
            raise ValueError(_NO_DSL_MC if not callable(test_fn) else
                             'dual_softmax: a callable test_fn computes its own metrics')
        self.gpu_collect, self.broadcast_bn_buffer, self.printer = gpu_collect, broadcast_bn_buffer, printer
        as_list = lambda k, d: list(d) if k is None else ([k] if isinstance(k, str) else list(k))          # noqa: E731
        self.greater_keys = as_list(greater_keys, self._default_greater_keys)
        self.less_keys = as_list(less_keys, self._default_less_keys)
        self.records, self.best_ckpt_path = [], None
        if self.save_best is not None:
            self._init_rule(rule, self.save_best)

    def _init_rule(self, rule, key_indicator):
        """:534-581 — without a rule: the key (case-insensitive) equal to, else containing, an entry of greater_keys /
        less_keys, greater first; 'auto' is resolved at the first evaluation from the first metric key."""
        if rule not in self.rule_map and rule is not None:
            raise KeyError(f'rule must be greater, less or None, but got {rule}.')
        if rule is None and key_indicator != 'auto':
            lc = key_indicator.lower()
            greater, less = [k.lower() for k in self.greater_keys], [k.lower() for k in self.less_keys]
            if lc in greater:
                rule = 'greater'
            elif lc in less:
                rule = 'less'
            elif any(k in lc for k in greater):
                rule = 'greater'
            elif any(k in lc for k in less):
                rule = 'less'
            else:
                raise ValueError(f'Cannot infer the rule for key {key_indicator}, thus a specific rule must be specified.')
        self.rule, self.key_indicator = rule, key_indicator
        if self.rule is not None:
            self.compare_func = self.rule_map[self.rule]

    @staticmethod
    def _rank_world():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    # ---- call points (:583-616)
    def before_run(self, runner):
        if self.save_best is not None:
            if runner.meta is None:
                runner.meta = {}
            runner.meta.setdefault('hook_msgs', {})
            self.best_ckpt_path = runner.meta['hook_msgs'].get('best_ckpt', None)

    def before_train_iter(self, runner):
        if self.by_epoch or not self.initial_flag:
            return
        if self.start is not None and runner.iter >= self.start:
            self.after_train_iter(runner)
        self.initial_flag = False

    def before_train_epoch(self, runner):
        if not (self.by_epoch and self.initial_flag):
            return
        if self.start is not None and runner.epoch >= self.start:
            self.after_train_epoch(runner)
        self.initial_flag = False

    def after_train_iter(self, runner):
        if not self.by_epoch:
            self._do_evaluate(runner)

    def after_train_epoch(self, runner):
        if self.by_epoch:
            self._do_evaluate(runner)

    def _should_evaluate(self, runner):
        """:631-664."""
        current = runner.epoch if self.by_epoch else runner.iter
        if self.start is None:
            return (current + 1) % self.interval == 0
        if (current + 1) < self.start:
            return False
        return (current + 1 - self.start) % self.interval == 0

    # ---- the evaluation itself (:843-878)
    @staticmethod
    def _guard(runner):
        """What an evaluation must leave alone: the model's mode, and on a CloverEngine the number of captured graph
        sets, the first-touch marks and the device counter the dropout seeds come from."""
        eng = runner.stepper
        state = dict(training=runner.model.training)
        if hasattr(eng, '_captures'):
            from . import ops
            state['captures'] = len(eng._captures)
            state['first_touch'] = (eng._ft.on, frozenset(eng._ft.done))
            dev = next(runner.model.parameters()).device
            if ops._dev_key(dev) in ops._DROPOUT_COUNTER:
                state['dropout_counter'] = int(ops._dropout_counter(dev).item())
        return state

    def _test(self, model):
        from .evaluation import (evaluate_qa, evaluate_retrieval, multi_gpu_test_itm_finetune,
                                 multi_gpu_test_retrieval, multi_gpu_test_retrieval_varied)
        rank, _ = self._rank_world()
        if callable(self.test_fn):
            res = self.test_fn(model, self.dataloader)
            return dict(res) if rank == 0 else None
        if self.test_fn == 'use_itm_head_fn':
            res = multi_gpu_test_itm_finetune(model, self.dataloader)
            return evaluate_qa(res, self.metrics) if rank == 0 else None
        if 'recall_for_video_text_retrieval_varied' in self.metrics:
            res = multi_gpu_test_retrieval_varied(model, self.dataloader, to_host=False)
        else:
            res = multi_gpu_test_retrieval(model, self.dataloader, gpu_collect=self.gpu_collect, to_host=False,
                                           with_label='video_qa_mc' in self.metrics)
        if rank != 0:
            return None
        opt = {} if self.dual_softmax is None else dict(dual_softmax=self.dual_softmax)
        return evaluate_retrieval(res, self.metrics, **opt)

    def _do_evaluate(self, runner):
        rank, world = self._rank_world()
        if self.broadcast_bn_buffer and world > 1:                    # :850-856, before the schedule check as there
            import torch.distributed as dist
            from .nn import BatchNorm1d
            for m in runner.model.modules():
                if isinstance(m, BatchNorm1d) and m.track_running_stats:
                    dist.broadcast(m.running_var, 0)
                    dist.broadcast(m.running_mean, 0)
        if not self._should_evaluate(runner):
            return
        before = self._guard(runner)
        eval_res = self._test(runner.model)
        after = self._guard(runner)
        if after != before:
            raise RuntimeError(f'EvalHook: the test loop disturbed the training state: {before} -> {after}')
        if rank != 0:
            return
        when = dict(epoch=runner.epoch + 1) if self.by_epoch else dict(iter=runner.iter + 1)
        rec = dict(when, mode='val', **{k: float(v) for k, v in eval_res.items()})
        if getattr(runner.stepper, 'ema_names', None):           # an engine with a weight EMA: which weights were scored
            rec['ema'] = bool(runner.stepper.ema_swapped)
        self.records.append(rec)
        if self.printer:
            self.printer(rec)
        if self.save_best:
            self._save_ckpt(runner, eval_res)

    def _save_ckpt(self, runner, eval_res):
        """:666-707 — compare, note best score and path in runner.meta['hook_msgs'], drop the previous best file, save."""
        current = f'epoch_{runner.epoch + 1}' if self.by_epoch else f'iter_{runner.iter + 1}'
        if self.key_indicator == 'auto':
            self._init_rule(self.rule, list(eval_res.keys())[0])
        key_score = eval_res[self.key_indicator]
        msgs = runner.meta.setdefault('hook_msgs', {})
        best_score = msgs.get('best_score', self.init_value_map[self.rule])
        if not self.compare_func(key_score, best_score):
            return
        msgs['best_score'] = float(key_score)
        if self.best_ckpt_path and os.path.isfile(self.best_ckpt_path):
            os.remove(self.best_ckpt_path)
        name = f'{os.path.basename(os.path.normpath(runner.work_dir))}_best_{self.key_indicator}_{current}.pth'
        self.best_ckpt_path = os.path.join(runner.work_dir, name)
        msgs['best_ckpt'] = self.best_ckpt_path
        runner.save_checkpoint(runner.work_dir, name)
        if self.printer:
            self.printer(f'Now best checkpoint is saved as {name}. Best {self.key_indicator} is '
                         f'{float(key_score):0.4f} at {current.replace("_", " ")}')


class BaseEMAHook(Hook):
    """``ema_hook`` (mmaction/core/hooks/ema.py:8-97): evaluation, best-checkpoint selection and every saved checkpoint
    use an exponential moving average of the weights, training goes on with the raw ones.

    The average lives in the engine (``CloverEngine.ema_enable`` / ``ema_update`` / ``ema_swap``: fp32 slabs, one HIP launch
    per update and per exchange) — this class is the schedule and the call points:

    * ``before_run``: ``ema_enable(skip_buffers)``, which registers the ``ema_*`` buffers, THEN ``runner.resume(resume_from)``
      if given, so that the checkpoint's ``ema_*`` entries find their buffers (:43-62);
    * ``after_train_iter``: an update with ``momentum_fun(runner.iter)`` (or ``momentum``) when
      ``(runner.iter + 1) % interval == 0`` — also after a step the loss scaler skipped, and once per loader step in the
      multi-loader runner, whose steps of one batch index share ``runner.iter`` (:68-79);
    * ``after_train_epoch`` / ``before_train_epoch``: exchange weights and average (:81-97).  The first epoch's exchange
      swaps equal values; it is what makes a resumed run work: a checkpoint written at an epoch's end holds the average in
      the parameters and the weights in ``ema_*``, and the first ``before_train_epoch`` after the resume puts them back.
      ``engine.ema_swapped`` says which way round they are: True from ``before_run`` and from every epoch's end until the
      next epoch begins (the engine refuses to train then), False during an epoch.

    Registered with priority 49 (``tools/train.py:220``) it runs ahead of ``CheckpointHook`` and ``EvalHook``."""

    def __init__(self, momentum=0.0002, interval=1, skip_buffers=False, resume_from=None, momentum_fun=None):
        assert 0 < momentum < 1
        self.momentum, self.interval, self.skip_buffers = momentum, interval, skip_buffers
        self.checkpoint, self.momentum_fun = resume_from, momentum_fun

    def before_run(self, runner):
        eng = runner.stepper
        missing = [a for a in ('ema_enable', 'ema_update', 'ema_swap') if not hasattr(eng, a)]
        if missing:
            raise TypeError(f'{type(self).__name__}: the weight EMA lives in the CloverEngine (its fp32 slabs and the 16-bit '
                            f'copies the kernels compute from); the stepper {type(eng).__name__} has no '
                            f'{", ".join(missing)} — drive the run with a CloverEngine')
        eng.ema_enable(skip_buffers=self.skip_buffers)
        if self.checkpoint is not None:
            runner.resume(self.checkpoint)
        # Until the first before_train_epoch the parameters COUNT as the average: after a resume they are it (see above),
        # at a fresh start average and weights are equal, so the label costs nothing — and the exchange that opens every
        # epoch, the first included, then leaves ``ema_swapped`` False while the engine trains.
        eng.ema_swapped = True

    def get_momentum(self, runner):
        return self.momentum_fun(runner.iter) if self.momentum_fun else self.momentum

    def after_train_iter(self, runner):
        if (runner.iter + 1) % self.interval != 0:
            return
        runner.stepper.ema_update(self.get_momentum(runner))

    def after_train_epoch(self, runner):
        runner.stepper.ema_swap()              # the average goes in ahead of EvalHook / CheckpointHook

    def before_train_epoch(self, runner):
        runner.stepper.ema_swap()              # ... and out again (at the first epoch: equal values, see above)


class ExpMomentumEMAHook(BaseEMAHook):
    """:100-111 — the momentum decays from ~1 towards ``momentum`` with time constant ``total_iter``."""

    def __init__(self, total_iter=2000, **kwargs):
        super().__init__(**kwargs)
        self.total_iter = total_iter
        self.momentum_fun = lambda x: (1 - self.momentum) * math.exp(-(1 + x) / total_iter) + self.momentum


class LinearMomentumEMAHook(BaseEMAHook):
    """:114-125 — ``momentum ** interval``, capped by ``(1 + x) / (warm_up + x)`` during the first iterations."""

    def __init__(self, warm_up=100, **kwargs):
        super().__init__(**kwargs)
        self.warm_up = warm_up
        self.momentum_fun = lambda x: min(self.momentum ** self.interval, (1 + x) / (warm_up + x))


EMA_HOOKS = {c.__name__: c for c in (BaseEMAHook, ExpMomentumEMAHook, LinearMomentumEMAHook)}

# mmcv's named priorities (mmcv/runner/priority.py): a lower value runs first
PRIORITIES = dict(HIGHEST=0, VERY_HIGH=10, HIGH=30, ABOVE_NORMAL=40, NORMAL=50, BELOW_NORMAL=60, LOW=70, VERY_LOW=90,
                  LOWEST=100)


def get_priority(priority):
    if isinstance(priority, str):
        return PRIORITIES[priority.upper()]
    if not isinstance(priority, int) or not 0 <= priority <= 100:
        raise ValueError(f'priority must be an integer in 0..100 or one of {sorted(PRIORITIES)}, got {priority!r}')
    return priority


class CloverRunner:
    """``stepper`` is a CloverEngine (``step(batch)``) or a module with ``train_step(batch, optimizer)``."""

    def __init__(self, stepper, model=None, optimizer=None, work_dir=None, max_epochs=None, meta=None):
        self.stepper = stepper
        self.model = model if model is not None else getattr(stepper, 'model', stepper)
        self.optimizer = optimizer
        self.work_dir, self.meta = work_dir, meta or {}
        self._max_epochs, self._max_iters = max_epochs, None
        self.epoch, self.iter, self.inner_iter = 0, 0, 0
        self.hooks, self.outputs, self.mode = [], None, None
        self.epoch_len = None                 # len(runner.data_loader): the longest loader in multi-loader mode

    def register_hook(self, hook, priority=50):
        """mmcv's ``register_hook``: hooks run in the order of their priority (lower first; names as in mmcv), hooks of
        equal priority in the order of their registration."""
        hook.priority = get_priority(priority)
        at = len(self.hooks)
        while at > 0 and getattr(self.hooks[at - 1], 'priority', 50) > hook.priority:
            at -= 1
        self.hooks.insert(at, hook)

    def call_hook(self, name):
        for h in self.hooks:
            getattr(h, name)(self)

    def run_iter(self, data_batch):
        if hasattr(self.stepper, 'step'):
            self.outputs = self.stepper.step(data_batch)
        else:
            self.outputs = self.stepper.train_step(data_batch, self.optimizer)
        if not isinstance(self.outputs, dict):
            raise TypeError('train_step must return a dict')            # epoch_based_runner run_iter

    # ---- clover_runner.py:17-35 (single loader)
    def _train_single(self, loader):
        self.epoch_len = len(loader)
        self._max_iters = self._max_epochs * len(loader)
        self.call_hook('before_train_epoch')
        for i, data_batch in enumerate(loader):
            self.inner_iter = i
            self.call_hook('before_train_iter')
            self.run_iter(data_batch)
            self.call_hook('after_train_iter')
            self.iter += 1
            if i >= len(loader) - 1:
                break
        self.call_hook('after_train_epoch')
        self.epoch += 1

    # ---- clover_runner.py:60-96 (several loaders; one optimizer step per loader per batch index)
    def _train_multi(self, loaders):
        self.epoch_len = max(len(ld) for ld in loaders)                # :62-69 — data_loader = the longest one
        self._max_iters = self._max_epochs * self.epoch_len
        self.call_hook('before_train_epoch')
        short_loader = None
        for batch_idx, batches in enumerate(zip_longest(*loaders)):
            self.inner_iter = batch_idx
            for loader_idx, data_batch in enumerate(batches):
                # :78-82 — the FIRST exhausted loader is restarted once, and from then on EVERY slot of the row
                # (also the longer loader's, whose own batch is dropped) is fed from that restarted iterator
                if short_loader is None and data_batch is None:
                    short_loader = iter(loaders[loader_idx])
                    data_batch = next(short_loader)
                elif short_loader is not None:
                    data_batch = next(short_loader)
                self.call_hook('before_train_iter')
                self.run_iter(data_batch)
                self.call_hook('after_train_iter')
            self.iter += 1                                   # :91 — counts batch indices, not optimizer steps
            if batch_idx >= max(len(ld) - 1 for ld in loaders):
                break
        self.call_hook('after_train_epoch')
        self.epoch += 1

    def train(self, data_loader, multi=False):
        """One epoch over a loader, or (multi=True) over a list of loaders interleaved."""
        self.model.train()
        self.mode = 'train'
        if multi:
            self._train_multi(list(data_loader))
        else:
            self._train_single(data_loader)

    def run(self, data_loaders, workflow=(('train', 1),), max_epochs=None):
        """clover_runner.py:98-163: workflow of ('train', n) phases until max_epochs; a list of loaders with a
        single ('train', n) entry is the multi-dataset mode."""
        if max_epochs is not None:
            self._max_epochs = max_epochs
        assert self._max_epochs is not None, 'max_epochs must be specified'
        self.call_hook('before_run')
        while self.epoch < self._max_epochs:
            for i, (mode, epochs) in enumerate(workflow):
                if mode != 'train':
                    raise ValueError(f'runner has no method named "{mode}" to run an epoch')
                for _ in range(epochs):
                    if self.epoch >= self._max_epochs:
                        break
                    multi = len(workflow) == 1 and len(data_loaders) > 1
                    self.train(data_loaders if multi else data_loaders[i], multi=multi)
        self.call_hook('after_run')

    # ---- checkpoints (epoch_based_runner.py:25-58 layout)
    def save_checkpoint(self, out_dir, filename):
        os.makedirs(out_dir, exist_ok=True)
        meta = dict(self.meta, epoch=self.epoch + 1, iter=self.iter, time=time.asctime())
        sd = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        ckpt = dict(meta=meta, state_dict=sd)
        if hasattr(self.stepper, 'optimizer_state'):
            ckpt['optimizer'] = self.stepper.optimizer_state()
        elif self.optimizer is not None:
            ckpt['optimizer'] = self.optimizer.state_dict()
        path = os.path.join(out_dir, filename)
        torch.save(ckpt, path)
        return path

    def load_checkpoint(self, path, strict=False):
        ckpt = torch.load(path, map_location='cpu')
        sd = ckpt.get('state_dict', ckpt)
        sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}        # DDP prefix
        res = self.model.load_state_dict(sd, strict=strict)
        if hasattr(self.stepper, 'refresh_shadow'):
            self.stepper.refresh_shadow()                # the engine computes from a bf16 copy of the weights
        return ckpt, res

    def resume(self, path):
        ckpt, _ = self.load_checkpoint(path)
        self.epoch = ckpt['meta'].get('epoch', 0)
        self.iter = ckpt['meta'].get('iter', 0)
        if 'optimizer' in ckpt and hasattr(self.stepper, 'load_optimizer_state'):
            self.stepper.load_optimizer_state(ckpt['optimizer'])
        # mmcv's resume: what hooks noted in the checkpoint (EvalHook: best_score / best_ckpt) carries over, so the
        # resumed run keeps comparing against the best score so far
        if ckpt['meta'].get('hook_msgs'):
            self.meta.setdefault('hook_msgs', {}).update(ckpt['meta']['hook_msgs'])
        return ckpt
