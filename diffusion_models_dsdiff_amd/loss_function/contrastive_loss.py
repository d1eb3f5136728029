"""ContrastiveLoss — drop-in for loss_function/contrastive_loss.py (forward only, on the device).

The supervised-contrastive loss of https://arxiv.org/pdf/2004.11362.pdf as the reference evaluates it for the disentangle heads:
``contrast_mode='all'`` with ``contrastive_method='cl'``.  The R x R x D broadcast the reference's CosineSimilarity materialises
is one pass of dsd_op_contrast_rows over the features (fp64 dot products), the loss its second kernel.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _sched


class ContrastiveLoss(nn.Module):
    def __init__(self, temperature=0.1, contrast_mode='all', base_temperature=0.1, contrastive_method='simclr'):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self.contrastive_method = contrastive_method

    def forward(self, features, labels=None, mask=None, temperature=None):
        """``features`` [bsz, n_views, ...] (CUDA), ``labels`` [bsz, n_views] -> (loss, logits [R,R], perfect_logit [R,R]),
        R = n_views*bsz rows ordered as torch.cat(torch.unbind(features, 1), 0).  Neither labels nor mask: the reference's eye
        mask [bsz,bsz], which fits its [R,R] logits with one view only."""
        if len(features.shape) < 3:
            raise ValueError('`features` needs to be [bsz, n_views, ...],'
                             'at least 3 dimensions are required')
        batch_size, n_views = features.shape[0], features.shape[1]
        if labels is not None and mask is not None:
            raise ValueError('Cannot define both `labels` and `mask`')
        if mask is not None:
            raise NotImplementedError("an explicit `mask` [bsz,bsz] is tiled nowhere in the reference (the 'tile mask' step is an "
                                      "empty comment, :102): it only fits the [R,R] logits when n_views is 1; pass `labels`")
        if self.contrast_mode == 'one':
            raise NotImplementedError("contrast_mode 'one' is broken in the reference: its [bsz,R] logits meet the [R,R] label mask "
                                      "and a scatter index of bsz rows (:104-112)")
        if self.contrast_mode != 'all':
            raise ValueError('Unknown mode: {}'.format(self.contrast_mode))
        if labels is not None and self.contrastive_method == 'infoNCE':
            raise NotImplementedError("contrastive_method 'infoNCE' is broken in the reference: cross_entropy over the raw features "
                                      "with relabelled classes (:66-77) fails unless D exceeds every label, and is unrelated to the logits")
        if labels is not None and self.contrastive_method != 'cl':
            # the reference leaves `mask` unset on this path and fails at torch.where (:81)
            raise ValueError('Unknown contrastive method: {}'.format(self.contrastive_method))
        if labels is None:
            if self.contrastive_method != 'cl':
                raise ValueError('Unknown contrastive method: {}'.format(self.contrastive_method))     # :134
            if n_views != 1:
                raise ValueError(f"without labels the mask is eye(bsz) = [{batch_size},{batch_size}] but the logits are "
                                 f"[{batch_size * n_views},{batch_size * n_views}]: the reference fails for n_views > 1")
            labels = torch.arange(batch_size).view(-1, 1)
        if labels.shape[0] != batch_size:
            raise ValueError('Num of labels does not match num of features')
        if not features.is_cuda:
            raise RuntimeError("ContrastiveLoss runs on the MI355X only (no CPU fallback): features are on the CPU")
        rows = _sched.label_rows(labels)
        t = self.temperature if temperature is None else temperature
        loss, logits = _sched.contrast_rows(torch.unbind(features, dim=1), rows, "cl", t)
        # (:120) the module's own temperature / base_temperature scales the loss whatever temperature the call passed
        loss = loss * (self.temperature / self.base_temperature)
        return loss, logits, _sched.perfect_logit(rows.to(features.device))
