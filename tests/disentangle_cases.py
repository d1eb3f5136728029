"""Shared by tests/golden/gen_disentangle.py, tests/test_disentangle_cpu.py and tests/test_disentangle_gpu.py: the cases of the
disentanglement-loss fixture (tests/golden/disentangle.npz), their inputs (regenerated from seeds: the fixture stores results
only) and a torch restatement of training_losses(disentangle=) (training_project/utils/gaussian_diffusion.py:907-975),
get_disentangle_loss (:1056-1094), ContrastiveLoss 'all' / 'cl' (loss_function/contrastive_loss.py) and the p = 1 distance of
trainers/trainer_ds_diff.py:341-354 that runs in fp32 or float64."""
import numpy as np
import torch

import loss_cases as LC
from oracle.synth import randn

TOL_OP = LC.TOL_OP                 # fp32 kernels against float64
TOL_NET = 5e-6                     # the bar the native features are held to (tests/test_loss_gpu.py, tests/test_disc_gpu.py)
NET_NOISE = 5e-6                   # relative size of the feature perturbation behind the fixture's sens_* entries (= TOL_NET)
MODES = ("contrast", "eu", "eu&contrast")          # training_losses(disentangle=)
METRICS = ("cl", "eu", "eu&cl", "l1")              # the op's
METRIC_OF = {"contrast": "cl", "eu": "eu", "eu&contrast": "eu&cl"}
T_CS, T_SAL = 0.05, 0.1                            # the temperatures of the two calls (:960-966)
LOSSES = ("disen_c_s_loss", "disen_s_a_l_loss")
MAPS = ("c_s_heatmap", "perfect_c_s_heatmap", "s_a_l_heatmap", "perfect_s_a_l_heatmap")
# (views, B, n): R = 6 and 7; odd n that is no multiple of 4; R = 112 over many slices with a ragged tail; the yaml network's
# head tensors at batch 16 (480 x 8 x 8, R = 96)
OP_SHAPES = ((6, 1, 20), (7, 1, 20), (6, 3, 256), (7, 3, 333), (7, 16, 4099), (6, 16, 30720))
STRIDED = (7, 3, 333)              # this case hands the op rows in a stride of n + 3
STUB_CASE = "tp_eps_fixed_mse"     # the rest of the stub-level call: a case of tests/loss_cases.py (B = 3)
STUB_FEAT = (32, 4, 4)
NET_NAMES = ("ds_tiny", "ds_tinyfilm")
HEADS = (("style", 3), ("content", 3), ("anatomy", 2), ("lesion", 2))


# ---------------------------------------------------------------------------------------------- labels
def cs_labels(B, n_content=3, n_style=3):
    """:932-937: [[0,0,0,-1,-2,-3],[1,1,1,-1,-2,-3],...]"""
    return np.array([[b] * n_content + [-1 - j for j in range(n_style)] for b in range(B)], dtype=np.int64)


def sal_labels(B, n_style=3, n_anatomy=2, n_lesion=2):
    """:940-951: [[-1,-2,-3,0,0,1,1],[-1,-2,-3,2,2,3,3],...]"""
    return np.array([[-1 - j for j in range(n_style)] + [2 * b] * n_anatomy + [2 * b + 1] * n_lesion for b in range(B)], dtype=np.int64)


def rows_of(label):
    """cat(unbind(label, 1), 0): row view*B + b."""
    return np.ascontiguousarray(np.asarray(label).T).reshape(-1)


def op_labels(views, B):
    return rows_of(cs_labels(B) if views == 6 else sal_labels(B))


# ---------------------------------------------------------------------------------------------- inputs
def op_views(views, B, n, seed=None):
    """``views`` fp32 CPU tensors [B, n]: a component shared by every row, one per sample and one per view beside unit noise, so
    that cosines spread over (0, 1) and no distance is degenerate."""
    seed = 12000 + 7 * views + 131 * B + n if seed is None else seed
    common, per_b, per_v = randn((1, 1, n), seed), randn((1, B, n), seed + 1), randn((views, 1, n), seed + 2)
    f = 0.5 * common + 0.5 * per_b + 0.4 * per_v + randn((views, B, n), seed + 3)
    return [f[v].contiguous() for v in range(views)]


def stub_feats(dtype=torch.float32):
    """The dict the stub model returns: DSUnetModel's head lists, B = 3."""
    B, k = LC.OP_B, 12500
    base = randn((B,) + STUB_FEAT, k)
    out = {}
    for name, cnt in HEADS:
        k += 10
        kind = randn((B,) + STUB_FEAT, k)
        out[name] = [(base + 0.7 * kind + 0.5 * randn((B,) + STUB_FEAT, k + 1 + i)).to(dtype) for i in range(cnt)]
    return out


# ---------------------------------------------------------------------------------------------- restatement
def _mask(rows):
    r = torch.as_tensor(np.asarray(rows)).view(-1, 1)
    return torch.eq(r, r.T)


def restate_cl(X, rows, temperature):
    """ContrastiveLoss(contrast_mode='all', contrastive_method='cl').forward in X's dtype (:98-131): (loss, logits)."""
    R = X.shape[0]
    norm = X.norm(dim=1).clamp_min(1e-8)                                  # CosineSimilarity(dim=-1), eps 1e-8
    logits = (X @ X.T) / (norm[:, None] * norm[None, :]) / temperature
    logits_mask = 1 - torch.eye(R, dtype=torch.float32)                    # (:63, :105: both masks are fp32 in any dtype, and so
    mask = _mask(rows).float() * logits_mask                              #  is the denominator mask.sum(1) + 1e-6 of :116)
    log_prob = logits - torch.log((torch.exp(logits) * logits_mask).sum(1, keepdim=True))
    mean_log_prob_pos = (mask * log_prob).sum(1) / (mask.sum(1) + 1e-6)
    return -(0.1 / 0.1) * mean_log_prob_pos.mean(), logits


def restate_ratio(logits, rows):
    mask = _mask(rows)
    eye = torch.eye(logits.shape[0], dtype=torch.bool)
    return torch.div((logits * ~eye * mask).sum(), (logits * ~mask).sum())


def restate(views, rows, metric, temperature, dtype=torch.float64):
    """(loss, the matrix the reference returns second) of ``views`` (tensors [B, ...]) in ``dtype``.  The Euclidean distance is
    float64 whatever the dtype and rounded to fp32 before the division by n, as :1065-1067 does; the distances are formed
    directly (no Gram matrix)."""
    X = torch.cat([v.reshape(v.shape[0], -1) for v in views], 0).to(dtype)
    n = X.shape[1]
    direct = "donot_use_mm_for_euclid_dist"
    if metric == "cl":
        return restate_cl(X, rows, temperature)
    if metric == "l1":
        logits = torch.cdist(X, X, p=1) / n
        return restate_ratio(logits, rows), logits
    if metric == "eu":
        logits = torch.cdist(X.double(), X.double(), p=2, compute_mode=direct).float() / n    # fp32 from here on in any dtype
        return restate_ratio(logits, rows).float(), logits * 2 - 1
    assert metric == "eu&cl"
    loss_con, logits_con = restate_cl(X, rows, temperature)
    logits = torch.cdist(X, X, p=2, compute_mode=direct) / n              # :1082: in the features' own dtype
    return restate_ratio(logits, rows) + 0.05 * loss_con, logits_con


def perfect(rows):
    return 2 * _mask(rows).float() - 1


def restate_terms(feats, mode, dtype=torch.float64):
    """The entries training_losses(disentangle=mode) adds for a feature dict (lists of [B, ...] tensors)."""
    B = feats["content"][0].shape[0]
    cs, sal = rows_of(cs_labels(B)), rows_of(sal_labels(B))
    l_cs, m_cs = restate(list(feats["content"]) + list(feats["style"]), cs, METRIC_OF[mode], T_CS, dtype)
    l_sal, m_sal = restate(list(feats["style"]) + list(feats["anatomy"]) + list(feats["lesion"]), sal, METRIC_OF[mode], T_SAL, dtype)
    return {"disen_c_s_loss": l_cs, "disen_s_a_l_loss": l_sal, "c_s_heatmap": m_cs, "perfect_c_s_heatmap": perfect(cs),
            "s_a_l_heatmap": m_sal, "perfect_s_a_l_heatmap": perfect(sal)}


def flat_terms(terms):
    """training_losses' dict with contrast_map's entries lifted beside the others, as float64 numpy."""
    out = {}
    for k, v in terms.items():
        for kk, vv in (v.items() if isinstance(v, dict) else ((k, v),)):
            out[kk] = vv.detach().double().cpu().numpy() if torch.is_tensor(vv) else np.asarray(vv, dtype=np.float64)
    return out


def dist(a, b):
    """Relative distance: of two scalars, or rel-L2 of two matrices / rows (float64)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))
