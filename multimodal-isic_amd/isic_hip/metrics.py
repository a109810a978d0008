"""Validation metrics from counts formed on the device.

The reference scores a validation set on the CPU with scikit-learn (``01_train_mil_teacher.py:111-113,266-272``,
``05_train_gnns.py:284-302``, ``utils_g_mil.py:245-251,806-812``).  Every metric it logs is a function of integers: the
confusion matrix and, per class, the number of (positive, negative) pairs the class score orders correctly, ties counting
half.  ``class_counts`` has ``isic_class_metrics_f32`` (include/isic_hip_metrics.h) form those integers and the fp64 loss
sum in one launch and reads them back in one small copy; ``ClassMetrics`` forms the floats from them in numpy fp64 on the
host, by the formulas sklearn 1.7.2 evaluates (tests/test_metrics_ref_cpu.py holds them to sklearn).
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from .lib import IsicHipError, call, header_path


def _header_constants():
    text = open(os.path.join(os.path.dirname(header_path()), "isic_hip_metrics.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+ISIC_METRICS_(BLOCK|TILE)\s+(\d+)", text)}


_CONST = _header_constants()
BLOCK, TILE = _CONST["BLOCK"], _CONST["TILE"]


def _mean(v, keep):
    return float(np.mean(v[keep])) if keep.any() else float("nan")


class ClassMetrics:
    """The metric set of the reference from ``confusion [C, C]`` (rows: label, columns: prediction), ``pair2 [C]`` and the
    loss sum.  ``n`` is the number of counted samples.

    ``accuracy``, ``bacc`` (mean recall over the classes with support), ``macro_precision`` / ``macro_recall`` /
    ``macro_f1`` (means over the classes that occur as a label or as a prediction: sklearn's label set, ``zero_division=0``),
    ``weighted_*`` (the same per-class values weighted by support), ``per_class_auc`` (NaN for a class without positives or
    without negatives), ``auc`` (the mean over all C classes: NaN as soon as one class has none, which is what
    ``roc_auc_score(..., multi_class="ovr", labels=arange(C))`` returns), ``loss`` (``loss_sum / n``; NaN without a loss).
    """

    def __init__(self, confusion, pair2, loss_sum=None):
        conf = np.asarray(confusion, dtype=np.int64)
        if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
            raise ValueError(f"confusion must be [C, C], got {conf.shape}")
        self.confusion = conf
        self.pair2 = np.asarray(pair2, dtype=np.int64).reshape(conf.shape[0])
        self.loss_sum = None if loss_sum is None else float(loss_sum)
        self.num_classes = C = conf.shape[0]
        self.n = n = int(conf.sum())
        tp = np.diag(conf).astype(np.float64)
        self.support = support = conf.sum(axis=1)
        self.predicted = predicted = conf.sum(axis=0)
        nan = float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            self.accuracy = float(tp.sum() / n) if n else nan
            recall = np.where(support > 0, tp / support, 0.0)
            precision = np.where(predicted > 0, tp / predicted, 0.0)
            f1 = np.where(precision + recall > 0, 2.0 * precision * recall / (precision + recall), 0.0)
            den = 2.0 * support.astype(np.float64) * (n - support).astype(np.float64)
            self.per_class_auc = np.where(den > 0, self.pair2.astype(np.float64) / den, np.nan)
        self.recall, self.precision, self.f1 = recall, precision, f1
        self.bacc = _mean(recall, support > 0)
        present = (support + predicted) > 0
        self.macro_precision, self.macro_recall, self.macro_f1 = (_mean(v, present) for v in (precision, recall, f1))
        w = support.astype(np.float64)
        self.weighted_precision, self.weighted_recall, self.weighted_f1 = (
            float((v * w).sum() / n) if n else nan for v in (precision, recall, f1))
        self.auc = float(np.mean(self.per_class_auc)) if C else nan
        self.loss = self.loss_sum / n if (self.loss_sum is not None and n) else nan

    def as_dict(self):
        """the keys ``evaluate_gnn`` returns"""
        return {"loss": self.loss, "accuracy": self.accuracy, "bacc": self.bacc, "auc": self.auc, "macro_f1": self.macro_f1}

    def __repr__(self):
        return (f"ClassMetrics(n={self.n}, accuracy={self.accuracy:.4f}, bacc={self.bacc:.4f}, auc={self.auc:.4f}, "
                f"macro_f1={self.macro_f1:.4f}, loss={self.loss:.4f})")


def _check(t, what, dtype, dim):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise IsicHipError(f"class_counts: {what} must be a device tensor (got a CPU tensor; there is no CPU fallback)")
    if t.dim() != dim or t.dtype != dtype:
        raise IsicHipError(f"class_counts: {what} must be a {dim}-D {dtype} tensor")
    return t.contiguous()


def class_counts_record(scores, labels, loss=None, out=None, workspace=None):
    """The launch alone: -> the int64 device record ``[C*C confusion | C pair2 | 2 flags | 1 loss sum (fp64 bits)]``.
    No synchronisation; ``out`` / ``workspace`` let a caller (a captured graph, a benchmark) own the buffers."""
    scores = _check(scores, "scores", torch.float32, 2)
    labels = _check(labels, "labels", torch.int64, 1)
    n, C = int(scores.shape[0]), int(scores.shape[1])
    if labels.shape[0] != n:
        raise ValueError(f"class_counts: {n} score rows, {labels.shape[0]} labels")
    if loss is not None:
        loss = _check(loss, "loss", torch.float32, 1)
        if loss.shape[0] != n:
            raise ValueError(f"class_counts: {n} score rows, {loss.shape[0]} losses")
    if out is None:
        out = torch.empty(C * C + C + 3, device=scores.device, dtype=torch.int64)
    nbytes = int(call("isic_class_metrics_f32_workspace_bytes", n, C))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 16), device=scores.device, dtype=torch.uint8)
    base, item = out.data_ptr(), 8
    call("isic_class_metrics_f32", scores if n else None, labels if n else None, loss if n else None, n, C, base,
         base + item * C * C, base + item * (C * C + C), base + item * (C * C + C + 2), workspace if nbytes else None,
         workspace.numel() if nbytes else 0)
    return out


def class_counts(scores, labels, loss=None):
    """``scores [n, C]`` fp32, ``labels [n]`` int64, ``loss [n]`` fp32 or None, all on the device -> ``ClassMetrics``.
    One launch of the entry and one host copy of ``C*C + C + 3`` words.  Raises ``ValueError`` when a score is NaN or
    infinite or a label lies outside ``[0, C)``, as sklearn does."""
    rec = class_counts_record(scores, labels, loss).cpu().numpy()
    C = int(scores.shape[1])
    conf, pair2 = rec[:C * C].reshape(C, C), rec[C * C:C * C + C]
    nonfinite, bad_labels = int(rec[C * C + C]), int(rec[C * C + C + 1])
    if nonfinite:
        raise ValueError(f"class_counts: scores contain NaN or infinity ({nonfinite} element(s))")
    if bad_labels:
        raise ValueError(f"class_counts: {bad_labels} label(s) outside the range [0, {C})")
    loss_sum = float(rec[C * C + C + 2:].view(np.float64)[0]) if loss is not None else None
    return ClassMetrics(conf, pair2, loss_sum)
