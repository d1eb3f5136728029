#!/usr/bin/env python3
"""Generate tests/golden/loss.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_loss.py

The reference's own GaussianDiffusion.training_losses — both copies: Disc_diff/guided_diffusion/gaussian_diffusion.py:821-920 and
training_project/utils/gaussian_diffusion.py:824- — on the cases of tests/loss_cases.py, every batch with mixed timesteps.

  ref cases   a stub model that returns stored tensors (the eight bottleneck tensors and the output for the Disc form; the
              output for the other); every case twice: as the reference computes it (fp32) and from the same reference code
              called on float64 tensors.
  net cases   the reference's own SuperResModelNew (UNet_disc_Model), DSUnetModel and UNetModel with the weights of disc.npz /
              model.npz / latent_ldm.npz.  The float64 twin of the DisC cases evaluates the network through tests/disc_ref.py
              (pinned to the reference by disc.npz: the reference's GroupNorm32 forces fp32), the loss through the reference.

              Also the 'hybrid' UNetModel of tests/cond_keys_util.py (its context reaches the network through the closure handed
              to training_losses, which passes c_concat only) and the small DiT, restated (tests/dit_loops_util.py, pinned to the
              reference's own DiT by dit.npz).
  p_losses    the reference's own DDPM.p_losses / get_loss / get_v and LatentDiffusion.p_losses (ldm/models/diffusion/ddpm.py:
              361-415, 892-927), imported through the stand-in finder of gen_trace.py (pytorch_lightning, omegaconf, ...) on a
              LatentDiffusion subclass without the constructor, as there.  Around a stub (fp32 and float64), and around the
              reference's DiffusionWrapper.forward over its own DSUnetModel, SuperResModelNew and UNetModel under 'concat',
              'crossattn', 'hybrid', 'adm', 'hybrid-adm' and 'crossattn-adm'.  LatentDiffusion.apply_model takes element 0 of a
              tuple; for SuperResModelNew's 9-tuple that is com_h1, not the prediction (the reference never runs that network
              under LatentDiffusion), so its case hands the wrapper the ninth element, as the reference's own samplers read it.

Stored: results only (every term, [B] each), the timesteps, and the measured gaps between the fp32 and the float64 runs.
Inputs regenerate from seeds (tests/loss_cases.py), weights from synth_params.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["DSD_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import loss_cases as LC  # noqa: E402
from gen_cfg import _params  # noqa: E402
import gen_trace as GT  # noqa: E402
from oracle.synth import synth_params  # noqa: E402

# the reference's training_project package is imported for real here; everything else gen_trace.py stands in for stays absent
GT.ABSENT = tuple(m for m in GT.ABSENT if m != "training_project")
sys.meta_path.insert(0, GT._Finder())

torch.set_grad_enabled(False)
torch.set_num_threads(8)


def ref_modules(form):
    # (training_project/utils/util.py imports cv2 and monai for the disentangle= path's heat maps, never run here: the finder's)
    if form == "disc":
        import Disc_diff.guided_diffusion.gaussian_diffusion as gd
        import Disc_diff.guided_diffusion.respace as rs
    else:
        import training_project.utils.gaussian_diffusion as gd
        import training_project.utils.respace as rs
    return gd, rs


def kwargs_of(form, planes):
    if form == "disc":
        return dict(t1=planes[0], t2=planes[1], dwi=planes[2])
    return dict(F_Data1=planes[0], F_Data2=planes[1], S_Data1=planes[2]) if len(planes) == 3 else dict(
        F_Data1=planes[0][:, :3], F_Data2=planes[0][:, 3:6], S_Data1=planes[0][:, 6:])


def run_ref(rc, model, x_start, noise, t, planes, dtype):
    gd, rs = ref_modules(rc["form"])
    d = LC.make_diffusion(gd, rs, rc)
    terms = d.training_losses(model, x_start.to(dtype), torch.from_numpy(t), model_kwargs=kwargs_of(rc["form"], [p.to(dtype) for p in planes]),
                              noise=noise.to(dtype))
    return {k: v.double().numpy() for k, v in terms.items() if torch.is_tensor(v)}


def gen_ref_cases(out, gaps):
    for name, rc in LC.REF_OP_CASES.items():
        inp = LC.ref_inputs(name)
        res = {}
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            o = inp["out"].to(dtype)
            fs = [f.to(dtype) for f in inp["feats"]]
            if rc["form"] == "disc":
                model = lambda x, ts, **kw: tuple(fs) + (o,)
            else:
                model = lambda x, ts, c_concat=None, **kw: o
            res[tag] = run_ref(rc, model, inp["x_start"], inp["noise"], inp["t"], inp["planes"], dtype)
        for k in res["32"]:
            out[f"ref_{name}_{k}"] = res["32"][k].astype(np.float32)
            out[f"ref64_{name}_{k}"] = res["64"][k]
            gaps.setdefault(k, []).append(LC.rel(res["32"][k], res["64"][k]))
        out[f"ref_{name}_keys"] = json.dumps(sorted(res["32"]))
        print(f"ref {name}: " + ", ".join(f"{k} {LC.rel(res['32'][k], res['64'][k]):.1e}" for k in sorted(res["32"])))


def cond_unet(name):
    """The reference's UNetModel of a tests/cond_keys_util.py model with that file's weights, and its conditioning key."""
    import cond_keys_util as U
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(**U.unet_params(name), use_checkpoint=False).eval()
    m.load_state_dict(synth_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], U.WEIGHT_SEED), strict=True)
    return m, U.MODELS[name][0]


def net_of(nc):
    g = np.load(os.path.join(HERE, nc["src"] + ".npz"), allow_pickle=False) if nc["src"] not in ("cond", "dit") else None
    if nc["src"] == "disc":
        from Disc_diff.guided_diffusion.unet import SuperResModelNew
        kw = json.loads(str(g[nc["key"] + "_cfg"]))
        sd = _params(g, nc["key"])
        m = SuperResModelNew(**kw, use_checkpoint=False).eval()
        m.load_state_dict(sd, strict=True)
        import disc_ref as R

        def m64(x, ts, **kwargs):
            return tuple(R.disc_forward(kw, sd, x.double(), ts, dtype=torch.float64))
        return (lambda x, ts, **kwargs: m(x, ts)), m64
    if nc["src"] == "model":
        from UNet_DS_Diff.model import DSUnetModel
        m = DSUnetModel(**json.loads(str(g[nc["key"] + "_cfg"])))
        m.load_state_dict(_params(g, nc["key"]), strict=True)
        m.eval()
        return (lambda x, ts, c_concat=None, **kw: m(torch.cat([x] + list(c_concat), 1), ts)[0]), None
    if nc["src"] == "dit":
        import dit_loops_util as DU
        return (lambda x, ts, c_concat=None, **kw: DU.oracle_net(nc["key"], torch.cat(list(c_concat), 1))(x, ts)), None
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    if nc["src"] == "cond":
        m, _ = cond_unet(nc["key"])
        return (lambda x, ts, c_concat=None, **kw: m(torch.cat([x] + list(c_concat), 1), ts, context=nc["ctx"])), None
    m = UNetModel(**json.loads(str(g["unet_cfg"])))
    m.load_state_dict(_params(g, "unet"), strict=True)
    m.eval()
    return (lambda x, ts, c_concat=None, **kw: m(torch.cat([x] + list(c_concat), 1), ts)), None


def gen_net_cases(out, gaps):
    for name, nc in LC.NET_CASES.items():
        x_start, planes, noise, t = LC.net_inputs(name)
        m32, m64 = net_of(dict(nc, ctx=LC.net_context(name)))
        r32 = run_ref(nc, m32, x_start, noise, t, planes, torch.float32)
        for k, v in r32.items():
            assert np.isfinite(v).all(), (name, k)
            out[f"net_{name}_{k}"] = v.astype(np.float32)
        out[f"net_{name}_keys"] = json.dumps(sorted(r32))
        out[f"net_{name}_t"] = t
        msg = ""
        if m64 is not None:
            r64 = run_ref(nc, m64, x_start, noise, t, planes, torch.float64)
            for k, v in r64.items():
                out[f"net64_{name}_{k}"] = v
                gaps.setdefault("net_" + k, []).append(LC.rel(r32[k], v))
            msg = f" gap {max(LC.rel(r32[k], r64[k]) for k in r32):.2e}"
        print(f"net {name}: " + ", ".join(f"{k} {v.mean():.5f}" for k, v in sorted(r32.items())) + msg)


def ldm_stand(ddpm_mod, par, kind, net, ckey):
    """LatentDiffusion without its constructor (gen_trace.py stand_in): register_schedule's defaults (linear, 1000 steps), the
    loss attributes of DDPM.__init__ (:106-132), the reference's DiffusionWrapper.forward over ``net`` as its model; eval mode."""
    class Wrap(ddpm_mod.DiffusionWrapper):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.sequential_cross_attn, self.conditioning_key = False, ckey
            self.diffusion_model = net

    class Stand(ddpm_mod.LatentDiffusion):
        device = torch.device("cpu")

        def __init__(self):
            torch.nn.Module.__init__(self)
            self.parameterization, self.v_posterior, self.num_timesteps_cond = par, 0., 1
            self.loss_type, self.learn_logvar = kind, False
            self.l_simple_weight, self.original_elbo_weight = LC.P_WEIGHTS["l_simple_weight"], LC.P_WEIGHTS["original_elbo_weight"]
            self.register_schedule()
            self.logvar = torch.full(fill_value=LC.P_WEIGHTS["logvar_init"], size=(self.num_timesteps,))
            self.model = Wrap()
    return Stand().eval()


class _Stub(torch.nn.Module):
    """A network that returns a stored tensor whatever it receives."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x, t, **kw):
        return self.out


class _Ninth(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, t):
        return self.m(x, t)[8]


def _scalars(d):
    return {k: np.float64(v.double().item()) for k, v in d.items()}


def gen_p_losses(out, gaps):
    ddpm_mod = GT.reference_ddpm()
    for name, (par, kind) in LC.P_STUB.items():
        c, inp = LC.p_stub_inputs(name)
        t = torch.from_numpy(inp["t"])
        res = {}
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            x_start, noise, o = (inp[k].to(dtype) for k in ("x_start", "noise", "out"))
            s = ldm_stand(ddpm_mod, par, kind, _Stub(o), None)
            r = {"ddpm/" + k: v for k, v in _scalars(ddpm_mod.DDPM.p_losses(s, x_start, t, noise=noise)[1]).items()}
            s.model.conditioning_key = "concat"
            s.model.diffusion_model = _Stub(o)
            r.update({"ldm/" + k: v for k, v in _scalars(s.p_losses(x_start, {"c_concat": [o]}, t, noise=noise)[1]).items()})
            target = LC.target_of(par, x_start, noise, inp["a"], inp["s"])
            r["get_loss_mean"] = np.float64(s.get_loss(o, target, mean=True).double().item())
            r["get_loss_rows"] = s.get_loss(o, target, mean=False).mean(dim=[1, 2, 3]).double().numpy()
            r["get_v"] = s.get_v(x_start, noise, t).double().numpy()
            res[tag] = r
        for k, v in res["32"].items():
            if k != "get_v":
                gaps.setdefault("p", []).append(LC.rel(v, res["64"][k]))
            out[f"p_{name}_{k}"] = np.asarray(v, dtype=np.float32)
            out[f"p64_{name}_{k}"] = np.asarray(res["64"][k])
        out[f"p_{name}_keys"] = json.dumps(sorted(res["32"]))
        print(f"p_losses stub {name}: gap {max(LC.rel(v, res['64'][k]) for k, v in res['32'].items()):.2e}")
    for name, pc in LC.P_NET.items():
        x_start, cond, noise, t = LC.p_net_inputs(name)
        if pc["src"] == "cond":
            net, _ = cond_unet(pc["key"])
        else:
            g = np.load(os.path.join(HERE, pc["src"] + ".npz"), allow_pickle=False)
            if pc["src"] == "disc":
                from Disc_diff.guided_diffusion.unet import SuperResModelNew
                net = SuperResModelNew(**json.loads(str(g[pc["key"] + "_cfg"])), use_checkpoint=False).eval()
            elif pc["src"] == "model":
                from UNet_DS_Diff.model import DSUnetModel
                net = DSUnetModel(**json.loads(str(g[pc["key"] + "_cfg"]))).eval()
            else:
                from ldm.modules.diffusionmodules.openaimodel import UNetModel
                net = UNetModel(**json.loads(str(g["unet_cfg"]))).eval()
            net.load_state_dict(_params(g, pc["key"]), strict=True)
            if pc["src"] == "disc":
                net = _Ninth(net)
        s = ldm_stand(ddpm_mod, pc["par"], pc["kind"], net, pc["ckey"])
        r = _scalars(s.p_losses(x_start, cond, t, noise=noise)[1])
        for k, v in r.items():
            assert np.isfinite(v), (name, k)
            out[f"pnet_{name}_{k}"] = np.float32(v)
        out[f"pnet_{name}_keys"] = json.dumps(sorted(r))
        print(f"p_losses net {name} ({pc['ckey']}): " + ", ".join(f"{k} {v:.5f}" for k, v in sorted(r.items())))
    out["p_stub"], out["p_net"] = json.dumps(LC.P_STUB), json.dumps(LC.P_NET)


def main():
    out, gaps = {}, {}
    gen_ref_cases(out, gaps)
    gen_net_cases(out, gaps)
    gen_p_losses(out, gaps)
    for k, v in gaps.items():
        out["gap_" + k] = np.float64(max(v))
        print(f"largest fp32-vs-float64 gap of the reference, {k}: {max(v):.3e}")
    out["gap_net"] = np.float64(max(max(v) for k, v in gaps.items() if k.startswith("net_")))
    out["gap_ref"] = np.float64(max(max(v) for k, v in gaps.items() if not k.startswith("net_")))
    out["ref_cases"], out["net_cases"] = json.dumps(LC.REF_OP_CASES), json.dumps(LC.NET_CASES)
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **out)
    print("wrote loss.npz:", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
