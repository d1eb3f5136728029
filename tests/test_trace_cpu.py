"""CPU side of the samplers' intermediates (tests/golden/trace.npz, tests/golden/gen_trace.py): the keep-set helper against the
iterations the reference kept, the ctypes mirror of dsd_trace and its export, fixture entries recomputed by the oracle networks
plus the chains of ddim.py / plms.py / ddpm.py restated in torch (which pins the fixture to the reference entry by entry), and the
restated make_grid."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import samplers as OS, schedules as S
from util import golden, rel_l2, randn
from test_img2img_cpu import blend, center_mask, guided
from test_plms_cpu import latent_env, plms_combine, norm_thresholding

TOL = 1e-5        # the bar of test_plms_cpu.py / test_img2img_cpu.py for their chains, here per entry
G = golden("trace")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases(space):
    """name -> dict(kind, steps, log, ...) of the fixture, with ``executed`` = the iterations the reference ran."""
    table = json.loads(str(G[space + "_cases"]))
    ex = json.loads(str(G[space + "_executed"]))
    return {k: dict(v, executed=ex[k]) for k, v in table.items()}


def entries(space, name, part):
    """The stored entries ``part`` ("x" / "p0") of a case, in order."""
    out, j = [], 0
    while f"{space}_{name}_{part}{j}" in G.files:
        out.append(torch.from_numpy(G[f"{space}_{name}_{part}{j}"]))
        j += 1
    return out


ALL = [(sp, n) for sp in ("lat", "pix") for n in cases(sp)]


# ---------------------------------------------------------------------------------------- the keep set, the ABI
def test_fixture_holds_the_cases_the_feature_is_specified_by():
    lat = cases("lat")
    assert {"ddim_log3", "ddim_log1", "ddim_log100", "ddim_eta1", "ddim_cfg", "ddim_mask", "ddim_v", "plms_log2", "plms_log2_thr",
            "ddpm_log5", "ddpm_log5_mask", "prog_log5"} <= set(lat)
    assert lat["ddim_log100"]["log"] == 100 and lat["ddim_v"]["param"] == "v" and lat["ddim_cfg"]["scale"] == float(G["scale"]) == 3.
    assert lat["ddpm_log5"]["steps"] == lat["prog_log5"]["steps"] == 12 and lat["plms_log2_thr"]["thr"] == float(G["thr"])
    assert lat["ddim_log3"]["executed"] == 8 and lat["plms_log2"]["executed"] == 7     # 'uniform': range(0, 1000, 1000 // S)


@pytest.mark.parametrize("space,name", ALL, ids=[f"{s}_{n}" for s, n in ALL])
def test_kept_iterations_are_the_reference_s(space, name):
    from diffusion_models_dsdiff_amd._sched import kept_iterations
    case = cases(space)[name]
    total = case["executed"]
    keep = G[f"{space}_{name}_keep"].tolist()
    assert kept_iterations(total, case["log"]) == keep
    assert keep[0] == 0 and keep[-1] == total - 1 and sorted(set(keep)) == keep
    # what the callbacks saw: DDIM / PLMS pass the iteration, the DDPM loops the timestep
    want = list(range(total)) if case["kind"] in ("ddim", "plms") else list(range(total - 1, -1, -1))
    assert G[f"{space}_{name}_cb"].tolist() == want and G[f"{space}_{name}_icb"].tolist() == want
    n = len(keep)
    assert len(entries(space, name, "x")) == (0 if case["kind"] == "prog" else n)
    assert len(entries(space, name, "p0")) == (0 if case["kind"] == "ddpm" else n)


def test_kept_iterations_edge_cases():
    from diffusion_models_dsdiff_amd._sched import kept_iterations
    assert kept_iterations(1, 100) == [0]
    assert kept_iterations(5, 1) == [0, 1, 2, 3, 4]
    assert kept_iterations(1000, 100) == [0] + [k for k in range(1000) if (999 - k) % 100 == 0]
    assert kept_iterations(6, 6) == [0, 5] and kept_iterations(7, 6) == [0, 6]


def test_trace_struct_mirrors_the_header():
    from diffusion_models_dsdiff_amd import _lib
    T = _lib.DsdTrace
    assert [f[0] for f in T._fields_] == ["keep", "n_keep", "x", "pred_x0"]
    assert (T.keep.offset, T.n_keep.offset, T.x.offset, T.pred_x0.offset) == (0, 8, 16, 24) and C.sizeof(T) == 32
    hdr = open(os.path.join(ROOT, "include", "dsdiff.h")).read()
    body = re.search(r"typedef struct dsd_trace \{(.*?)\} dsd_trace;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["keep", "n_keep", "x", "pred_x0"]
    assert "dsd_set_trace" in _lib.EXPORTS
    assert re.search(r"int dsd_set_trace\(dsd_handle\* h, const dsd_trace\* t\);", hdr)


# ---------------------------------------------------------------------------------------- restated chains, entry by entry
def _tables(od, S_):
    ts = S.make_ddim_timesteps("uniform", S_, od.num_timesteps)
    sig, a, a_prev = S.make_ddim_sampling_parameters(od.tab["alphas_cumprod"].numpy(), ts, 0.)
    return ts, sig, a, a_prev, np.sqrt(1. - a)


def ddim_trace_chain(od, f, img, S_, keep, clip=True):
    """ddim_sampling :156-183 + p_sample_ddim :221-260 at eta 0 -> (x entries, pred_x0 entries) of the iterations ``keep``."""
    ts, sig, a, a_prev, s1m = _tables(od, S_)
    b, total = img.shape[0], ts.shape[0]
    full = lambda v: torch.full((b, 1, 1, 1), float(v))
    xs, p0s = [], []
    for k, step in enumerate(np.flip(ts)):
        index = total - k - 1
        t = torch.full((b,), int(step), dtype=torch.long)
        e_t = f(img, t)
        x0 = (img - full(s1m[index]) * e_t) / full(a[index]).sqrt()
        if clip:
            x0 = x0.clamp(-1., 1.)
        img = full(a_prev[index]).sqrt() * x0 + (1. - full(a_prev[index]) - full(sig[index]) ** 2).sqrt() * e_t
        if k in keep:
            xs.append(img)
            p0s.append(x0)
    return xs, p0s


def plms_trace_chain(od, f, img, S_, keep, thr=None):
    """plms_sampling :147-176 + p_sample_plms :206-245 -> (x entries, pred_x0 entries): pred_x0 is the one of the step's final
    get_x_prev_and_pred_x0, after norm_thresholding."""
    ts, sig, a, a_prev, s1m = _tables(od, S_)
    time_range, total, b = np.flip(ts), ts.shape[0], img.shape[0]
    full = lambda v: torch.full((b, 1, 1, 1), float(v))
    old, xs, p0s = [], [], []

    def upd(x, e, index):
        p0 = (x - full(s1m[index]) * e) / full(a[index]).sqrt()
        if thr is not None:
            p0 = norm_thresholding(p0, thr)
        return full(a_prev[index]).sqrt() * p0 + (1. - full(a_prev[index])).sqrt() * e, p0
    for i, step in enumerate(time_range):
        index = total - i - 1
        t = torch.full((b,), int(step), dtype=torch.long)
        t_next = torch.full((b,), int(time_range[min(i + 1, total - 1)]), dtype=torch.long)
        e_t = f(img, t)
        e_next = f(upd(img, e_t, index)[0], t_next) if not old else None
        img, p0 = upd(img, plms_combine(e_t, old, e_next), index)
        old.append(e_t)
        if len(old) >= 4:
            old.pop(0)
        if i in keep:
            xs.append(img)
            p0s.append(p0)
    return xs, p0s


def ddpm_trace_chain(od, f, img, z, zb, x0, mask, timesteps, keep, clip=False):
    """p_sample_loop :1075-1092 / progressive_denoising :1024-1044 with p_sample(return_x0=True) -> (x entries after the blend,
    x_recon entries)."""
    T, e = od.tab, od._ext
    b = img.shape[0]
    xs, p0s = [], []
    for k, i in enumerate(reversed(range(timesteps))):
        t = torch.full((b,), i, dtype=torch.long)
        xr, _ = od.x0_eps(img, t, f(img, t))
        if clip:
            xr = xr.clamp(-1., 1.)
        mean = e(T["posterior_mean_coef1"], t, img.shape) * xr + e(T["posterior_mean_coef2"], t, img.shape) * img
        nz = (1 - (t == 0).float()).reshape(b, 1, 1, 1)
        img = mean + nz * (0.5 * e(T["posterior_log_variance_clipped"], t, img.shape)).exp() * z[k]
        if mask is not None:
            img = blend(od, x0, mask, t, zb[k], img)
        if k in keep:
            xs.append(img)
            p0s.append(xr)
    return xs, p0s


def _check(space, name, part, got):
    want = entries(space, name, part)
    assert len(got) == len(want) > 0
    for j, (a, b) in enumerate(zip(got, want)):
        err = rel_l2(a, b)
        print(f"{space}_{name} {part}{j}: rel-L2 to the reference {err:.3e}")
        assert err < TOL, (space, name, part, j, err)


def test_restated_chains_reproduce_the_reference_entries():
    _, net, c, u, xT = latent_env()
    assert int(golden("plms")["lat_xT_seed"]) == int(G["lat_xT_seed"]) and int(golden("plms")["lat_c_seed"]) == int(G["lat_c_seed"])
    od = OS.DiffusionB(timesteps=1000, parameterization="eps")
    table = cases("lat")
    # guided DDIM
    case, keep = table["ddim_cfg"], G["lat_ddim_cfg_keep"].tolist()
    xs, p0s = ddim_trace_chain(od, guided(net, c, u, case["scale"]), xT.clone(), case["steps"], keep)
    _check("lat", "ddim_cfg", "x", xs)
    _check("lat", "ddim_cfg", "p0", p0s)
    # thresholded PLMS
    case, keep = table["plms_log2_thr"], G["lat_plms_log2_thr_keep"].tolist()
    xs, p0s = plms_trace_chain(od, guided(net, c, u, 1.), xT.clone(), case["steps"], keep, thr=case["thr"])
    _check("lat", "plms_log2_thr", "x", xs)
    _check("lat", "plms_log2_thr", "p0", p0s)
    # masked DDPM and the progressive chain over the same 12 steps
    T = table["ddpm_log5_mask"]["steps"]
    shape = tuple(xT.shape)
    z, zb = randn((T,) + shape, int(G["step_seed"])), randn((T,) + shape, int(G["blend_seed"]))
    x0, mask = randn(shape, int(G["x0_seed"])), center_mask(shape)
    f = guided(net, c, u, 1.)
    xs, _ = ddpm_trace_chain(od, f, xT.clone(), z, zb, x0, mask, T, G["lat_ddpm_log5_mask_keep"].tolist())
    _check("lat", "ddpm_log5_mask", "x", xs)
    xs, p0s = ddpm_trace_chain(od, f, xT.clone(), z, None, None, None, T, G["lat_prog_log5_keep"].tolist())
    _check("lat", "prog_log5", "p0", p0s)
    assert rel_l2(xs[-1], G["lat_prog_log5_y"]) < TOL


# ---------------------------------------------------------------------------------------- the restated make_grid
@pytest.mark.parametrize("n,c,h,w,nrow", [(6, 1, 5, 7, 3), (4, 3, 4, 4, 4), (5, 1, 3, 3, 2)])
def test_make_grid_restatement(n, c, h, w, nrow):
    from diffusion_models_dsdiff_amd.ldm.util import make_grid
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(n * 10 + c))
    g = make_grid(x, nrow=nrow)
    cols = min(nrow, n)
    rows = -(-n // cols)
    assert tuple(g.shape) == (3, rows * (h + 2) + 2, cols * (w + 2) + 2)
    covered = torch.zeros_like(g, dtype=torch.bool)
    for k in range(n):
        r, q = divmod(k, cols)
        ys, xs = r * (h + 2) + 2, q * (w + 2) + 2
        cell = g[:, ys:ys + h, xs:xs + w]
        assert torch.equal(cell, x[k].expand(3, h, w) if c == 1 else x[k])      # every cell equals its input
        covered[:, ys:ys + h, xs:xs + w] = True
    assert torch.all(g[~covered] == 0)                                         # the padding (and the unused cells) are zero
    assert (~covered).any()


def test_make_grid_single_image_and_denoise_grid_layout():
    from diffusion_models_dsdiff_amd.ldm.util import denoise_grid, make_grid
    x = torch.randn(1, 1, 4, 4)
    assert torch.equal(make_grid(x), x[0].expand(3, 4, 4))                     # one image: returned as it is, three channels
    samples = [torch.full((2, 1, 3, 3), float(10 * j)) + torch.arange(2.).reshape(2, 1, 1, 1) for j in range(4)]   # n=4 entries, b=2
    g = denoise_grid(samples)
    assert tuple(g.shape) == (3, 2 * 5 + 2, 4 * 5 + 2)                         # one row per sample, one column per entry
    for b in range(2):
        for j in range(4):
            assert torch.all(g[:, b * 5 + 2:b * 5 + 5, j * 5 + 2:j * 5 + 5] == 10 * j + b)
