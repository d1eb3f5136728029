"""instantiate_from_config / get_obj_from_str — drop-in for ldm/util.py:82-97.

The yaml ``target:`` strings of the reference (e.g. ``UNet_DS_Diff.model.DSUnetModel``) resolve to the
native classes of this package, so the reference's model yamls work unchanged.
"""
import importlib

_PKG = __name__.split(".")[0]
# reference dotted paths served natively
_NATIVE_PREFIXES = ("UNet_DS_Diff.model", "ldm.util", "ldm.models.diffusion.ddpm", "ldm.models.diffusion.ddim",
                    "Disc_diff.guided_diffusion", "trainers.trainer_ddpm", "ldm.modules.diffusionmodules.openaimodel",
                    "ldm.models.autoencoder")


def exists(x):
    return x is not None


def default(val, d):
    if exists(val):
        return val
    return d() if callable(d) and not isinstance(d, type) else d


def get_obj_from_str(string, reload=False):
    module, cls = string.rsplit(".", 1)
    if any(module == p or module.startswith(p + ".") for p in _NATIVE_PREFIXES):
        module = _PKG + "." + module
    module_imp = importlib.import_module(module)
    if reload:
        importlib.reload(module_imp)
    return getattr(module_imp, cls)


def instantiate_from_config(config):
    if "target" not in config:
        if config == "__is_first_stage__":
            return None
        elif config == "__is_unconditional__":
            return None
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(config["target"])(**config.get("params", dict()))


def make_grid(tensor, nrow=8, padding=2, pad_value=0.):
    """torchvision.utils.make_grid at its documented defaults, restated (parity unpinned: torchvision is not a dependency of
    this package and no run of it stands behind this): [N,C,H,W] -> one [3 or C, rows*(H+padding)+padding, cols*(W+padding)+padding]
    image, ``nrow`` images per row, cell (r, c) at offset (r*(H+padding)+padding, c*(W+padding)+padding), the padding filled with
    ``pad_value``, no normalisation, one-channel images repeated to three channels; a single image comes back as it is."""
    import math

    import torch
    if tensor.dim() != 4:
        raise ValueError(f"make_grid takes [N,C,H,W], got {tuple(tensor.shape)}")
    if tensor.shape[1] == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    n, c, h, w = tensor.shape
    if n == 1:
        return tensor.squeeze(0)
    cols = min(int(nrow), n)
    rows = int(math.ceil(n / cols)) if cols else 0
    ch, cw = h + padding, w + padding
    grid = tensor.new_full((c, ch * rows + padding, cw * cols + padding), pad_value)
    for k in range(n):
        r, q = divmod(k, cols)
        grid[:, r * ch + padding:r * ch + padding + h, q * cw + padding:q * cw + padding + w] = tensor[k]
    return grid


def denoise_grid(samples):
    """_get_rows_from_list (trainers/trainer_ddpm.py:473-478; ldm/models/diffusion/ddpm.py:653-658): a list of n [b,c,h,w] entries
    -> the grid with one row per sample and one column per entry.  Parity unpinned, as make_grid."""
    import torch
    stack = torch.stack(list(samples))                                       # n b c h w
    n = stack.shape[0]
    return make_grid(stack.transpose(0, 1).reshape((stack.shape[1] * n,) + tuple(stack.shape[2:])), nrow=n)


def load_unet_from_yaml(path, **overrides):
    """Build the U-Net named by ``model.params.unet_config`` of a reference model yaml (PyYAML; the hot-path
    yamls use no OmegaConf interpolation — SURVEY.md 5)."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    uc = dict(cfg["model"]["params"]["unet_config"])
    uc["params"] = {**uc.get("params", {}), **overrides}
    return instantiate_from_config(uc), cfg
