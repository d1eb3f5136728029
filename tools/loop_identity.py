#!/usr/bin/env python3
"""Before / after identity of the device loops: what every loop computes through the Python API (which a refactor of the C entry
points leaves alone), as a JSON of SHA-256 digests that two checkouts can be compared on case by case.

    python tools/loop_identity.py --out a.json        # in a checkout of the other commit, a fresh process
    python tools/loop_identity.py --out b.json        # in this one
    python tools/loop_identity.py --compare a.json b.json [--json verdict.json]

Each commit runs from its own checkout with its own library: DSD_LIBRARY cannot stand in for the checkout, because a library from
before the loops took one entry point each no longer matches the binding's loop signatures.

Cases, each on the tiny DSUnetModel of tests/golden/model.npz (pix) and the UNetModel of tests/golden/latent_ldm.npz (lat), with
host launches (graph0) and with graph replay (graph1): DDIM (eta 1) and DDPM with fed noise, Philox noise and a first_step split;
guided DDIM (per-step scales 1.5 .. 3.5); masked B_DDIM, guided masked B_DDIM and masked B_DDPM, blend noise fed and Philox, split;
DPM-Solver++ order 2 plain and guided; the DPM program (singlestep 3, multistep 3, with kept states); PLMS plain, thresholded,
guided + masked, guided split, masked with Philox blend noise; DDIM inversion plain, guided, guided split; the variational bound.
One DiT (M1 of tests/dit_loops_util.py) and one DisC-Diff network (`tiny` of tests/golden/disc.npz) run a DDIM loop each.
dsd_graph_stats of every handle is recorded after each pass."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS, SPLIT = 8, 3


def compare(pa, pb, out):
    a, b = json.load(open(pa)), json.load(open(pb))
    names = sorted(set(a["cases"]) | set(b["cases"]))
    cases = {k: k in a["cases"] and a["cases"].get(k) == b["cases"].get(k) for k in names}
    verdict = {"a": a["commit"], "b": b["commit"], "n_cases": len(cases), "cases": cases,
               "graph_stats": {"a": a["graph_stats"], "b": b["graph_stats"], "equal": a["graph_stats"] == b["graph_stats"]}}
    verdict["all_equal"] = bool(cases) and all(cases.values()) and verdict["graph_stats"]["equal"]
    for k, ok in cases.items():
        if not ok:
            print("DIFFERENT", k)
    print(f"{len(cases)} cases, graph_stats equal = {verdict['graph_stats']['equal']}, all_equal = {verdict['all_equal']}")
    if out:
        json.dump(verdict, open(out, "w"), indent=1)
    return 0 if verdict["all_equal"] else 1


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
ap.add_argument("--json")
ap.add_argument("--commit", default="", help="label stored in the output (the commit the checkout is at)")
args = ap.parse_args()
if args.compare:
    sys.exit(compare(args.compare[0], args.compare[1], args.json))

import numpy as np
import torch
from diffusion_models_dsdiff_amd import _lib
from diffusion_models_dsdiff_amd._sched import (Guidance, Inpaint, Schedule, run_bpd_loop, run_device_loop, run_invert_loop,
                                                run_plms_loop, invert_coefficients)
from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper, LatentDiffusion
from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
from util import golden, fixture_params, randn, cond_image
import dit_loops_util as U
import disc_ref as R

_lib.require_gpu(0)
CASES, STATS = {}, {}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().float().cpu().numpy()).tobytes())
    return h.hexdigest()


def pix_env():
    gm = golden("model")
    wrap = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
    wrap.diffusion_model.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    m = DDPMModel(timesteps=1000, parameterization="v").cuda()
    m.model = wrap
    shape = (2, 1, 32, 32)
    return dict(m=m, wrap=wrap, unet=wrap.diffusion_model, c=cond_image(shape, 11).cuda(), xT=randn(shape, 12).cuda(),
                x0=randn(shape, 13).cuda())


def lat_env():
    gl = golden("latent_ldm")
    dd = json.loads(str(gl["vae_cfg"]))
    embed = dd.pop("embed_dim")
    ld = LatentDiffusion(first_stage_config=AutoencoderKL(dd, None, embed), conditioning_key="concat", scale_factor=0.18215,
                         timesteps=1000, parameterization="v", image_size=8, channels=4,
                         unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                                      "params": json.loads(str(gl["unet_cfg"]))})
    ld.model.diffusion_model.load_state_dict(fixture_params(gl, "unet"), strict=True)
    ld = ld.cuda()
    shape = (2, 4, 8, 8)
    return dict(m=ld, wrap=ld.model, unet=ld.model.diffusion_model, c=randn((2, 8, 8, 8), 21).cuda(), xT=randn(shape, 22).cuda(),
                x0=randn(shape, 23).cuda())


def split(run):
    """A loop in two calls: iterations [0, SPLIT), then the rest from the state the first call returned."""
    return run(run(None, 0, SPLIT), SPLIT, 0)


def loops(tag, e, ddpm):
    unet, xT, c, x0 = e["unet"], e["xT"], e["c"], e["x0"]
    u = torch.zeros_like(c)
    mask = torch.zeros_like(xT[:, :1])
    mask[:, :, : xT.shape[2] // 2] = 1.
    z, zb = randn((STEPS,) + tuple(xT.shape), 31).cuda(), randn((STEPS,) + tuple(xT.shape), 32).cuda()
    guid = lambda n=STEPS: Guidance(u, np.linspace(1.5, 3.5, n), n)
    put = lambda name, *t: CASES.__setitem__(f"{tag}_{name}", digest(*t))
    s = DDIMSampler(e["m"])
    s.make_schedule(STEPS, ddim_eta=1.0, verbose=False)
    ddim = s._schedule(False, True)

    def family(name, sched, **kw):
        """fed noise, Philox noise, and the Philox run split at SPLIT."""
        fed = dict(kw, inpaint=Inpaint(x0, mask, zb)) if "inpaint" in kw else kw
        put(name + "_fed", run_device_loop(unet, sched, xT, c, step_noise=z, **fed))
        put(name + "_philox", run_device_loop(unet, sched, xT, c, seed=5, **kw))
        put(name + "_split", split(lambda x, k0, n: run_device_loop(unet, sched, xT if x is None else x, c, seed=5, first_step=k0,
                                                                    n_steps=n, **kw)))
    family("sample_ddim", ddim)
    family("sample_ddpm", ddpm)
    family("guided", ddim, guidance=guid())
    family("masked_ddim", ddim, inpaint=Inpaint(x0, mask))
    family("masked_ddim_guided", ddim, inpaint=Inpaint(x0, mask), guidance=guid())
    family("masked_ddpm", ddpm, inpaint=Inpaint(x0, mask))
    # DPM-Solver: the order <= 2 loop and the program
    ns = dsa.NoiseScheduleVP("discrete", betas=e["m"].betas.detach().float().cpu())
    fn = dsa.model_wrapper(e["wrap"], ns, model_type="v", model_kwargs=dict(c_concat=[c]))
    sol = dsa.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    sched = sol.build_schedule(steps=STEPS, order=2, skip_type="logSNR", lower_order_final=True, denoise_to_zero=True)
    put("dpm", dsa.run_dpm_loop(fn, sched, xT))
    put("dpm_guided", dsa.run_dpm_loop(fn, sched, xT, Guidance(u, 3.0, sched.steps)))
    for name, method in (("ss3", "singlestep"), ("ms3", "multistep")):
        prog = sol.build_program(steps=9, order=3, skip_type="logSNR", method=method, return_intermediate=True)
        put("dpm_program_" + name, *dsa.run_dpm_program(fn, prog, xT))
        put("dpm_program_" + name + "_guided", *dsa.run_dpm_program(fn, prog, xT, Guidance(u, 3.0, prog.steps)))
    # PLMS
    keep, e["m"].parameterization = e["m"].parameterization, "eps"           # PLMS takes the output as a noise prediction
    p = PLMSSampler(e["m"])
    p.make_schedule(STEPS, verbose=False)
    plms = p._schedule()
    e["m"].parameterization = keep
    put("plms", run_plms_loop(unet, plms, xT, c))
    put("plms_thr", run_plms_loop(unet, plms, xT, c, threshold=0.5))
    put("plms_guided_masked_fed", run_plms_loop(unet, plms, xT, c, threshold=0.5, guidance=guid(), inpaint=Inpaint(x0, mask, zb)))
    put("plms_guided_split", split(lambda x, k0, n: run_plms_loop(unet, plms, xT if x is None else x, c, guidance=guid(),
                                                                   first_step=k0, n_steps=n)))
    put("plms_masked_philox", run_plms_loop(unet, plms, xT, c, inpaint=Inpaint(x0, mask), seed=6))
    # DDIM inversion (the coefficients DDIMSampler.encode forms)
    coef = invert_coefficients(torch.from_numpy(np.asarray(s.ddim_alphas[:STEPS], dtype=np.float32)),
                               torch.tensor(np.asarray(s.ddim_alphas_prev[:STEPS], dtype=np.float64)))
    put("invert", run_invert_loop(unet, coef, x0, c))
    put("invert_guided", run_invert_loop(unet, coef, x0, c, guid()))
    put("invert_guided_split", split(lambda x, k0, n: run_invert_loop(unet, coef, x0 if x is None else x, c, guid(), first_step=k0,
                                                                       n_steps=n)))
    # the variational bound
    d = create_gaussian_diffusion(steps=1000, timestep_respacing=str(STEPS), parameterization="v")
    res = run_bpd_loop(unet, d._schedule(False, 0.0, True), d._post_log_var(), float(d.log_one_minus_alphas_cumprod[-1]),
                       (0.5 * x0).clamp(-1, 1), c, seed=7)
    put("bpd", *[res[k] for k in ("vb", "xstart_mse", "mse", "prior_bpd")])


def one_ddim(tag, unet, xT, c):
    sched = create_gaussian_diffusion(steps=1000, timestep_respacing=str(STEPS))._schedule(True, 0.5, True)
    CASES[tag + "_ddim_philox"] = digest(run_device_loop(unet, sched, xT, c, seed=9))
    CASES[tag + "_ddim_fed"] = digest(run_device_loop(unet, sched, xT, c, step_noise=randn((STEPS,) + tuple(xT.shape), 41).cuda()))


pix, lat = pix_env(), lat_env()
keep, lat["m"].parameterization = lat["m"].parameterization, "eps"       # B_DDPM rows of an eps-model: the tables are the betas' alone
ddpm = lat["m"]._schedule(STEPS)
lat["m"].parameterization = keep
dit = DiffusionWrapper({"target": U.DIT_TARGET, "params": U.MODELS["M1"][0]}, "concat").diffusion_model
dit.load_state_dict(U.weights("M1"), strict=True)
dit_x, dit_c = (t.cuda() for t in U.inputs("M1", 2))
kw, sd, x, _ = R.case("tiny")
disc = DDPMModel(unet_config={"target": "Disc_diff.guided_diffusion.unet.SuperResModelNew", "params": kw}, conditioning_key="concat",
                 timesteps=1000, parameterization="eps").cuda().model.diffusion_model
disc.load_state_dict(sd, strict=True)
disc_x, disc_c = randn((2, 1) + tuple(x.shape[2:]), 51).cuda(), randn((2, 3) + tuple(x.shape[2:]), 52).cuda()
for graph in (0, 1):
    for name, net in (("pix", pix["unet"]), ("lat", lat["unet"]), ("dit", dit), ("disc", disc)):
        net.use_graph(bool(graph))
    loops(f"pix_graph{graph}", pix, ddpm)
    loops(f"lat_graph{graph}", lat, ddpm)
    one_ddim(f"dit_graph{graph}", dit, dit_x, dit_c)
    one_ddim(f"disc_graph{graph}", disc, disc_x, disc_c)
    for name, net in (("pix", pix["unet"]), ("lat", lat["unet"]), ("dit", dit), ("disc", disc)):
        st = net.graph_stats()
        STATS[f"{name}_graph{graph}"] = [st["captures"], st["launches"]]
torch.cuda.synchronize()
json.dump({"commit": args.commit, "cases": CASES, "graph_stats": STATS}, open(args.out, "w"), indent=1)
print(f"{len(CASES)} cases -> {args.out}")
