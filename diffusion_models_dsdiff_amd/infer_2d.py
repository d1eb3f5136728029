"""infer_2d — counterpart of the reference's inference/inference_2d_*.py entry scripts for the native path.

Reads the SAME yaml keys (model yaml: ``model.params.{unet_config, parameterization, …}``; inference yaml:
``sampler_setting.{sampler, sample_steps, ddim_eta, ddim_use_original_steps}``, ``test_batch_size``, ``seed``,
``cuda_idx`` — configs/inference_config_BraTs.yaml:11-19 of the reference).  Slices come either as one ``.npy``
``[N,C,H,W]`` (C = 1 or 3 condition channels) or as the reference's own slice files: ``--input <dir>`` with
``<dir>/<id>/<name>_<slice>.h5`` (preprocess/to_h5.py) and ``--input-keys`` naming the datasets used as condition channels
(h5lite.py reads them; no h5py).  Either way they are taken as already scaled to [-1,1] and sized to a multiple of 32, which
the reference does in its MONAI transform chain (not rebuilt).  Output: ``[N,1,H,W]`` as ``.npy``, or — with an h5 input
and ``--output <dir>`` — one NIfTI volume per id, the slices stacked at their index as on_predict_end does
(trainer_use_gaussian_diff.py:632-655; host_io.VolumeAssembler / write_nifti):
  * ``--template-dir <dir>``: ``<dir>/<id>/<template-name>`` (default name: the last input key + ".nii.gz", as the trainer's
    ``self.keys[-1] + ".nii.gz"``) is read, the prediction is ``zeros_like(template)`` with the predicted slices written at
    their index (trailing unpredicted slices stay zero, dtype = the template's), and it is saved with the template's header
    bytes (the role of ``pred_nii.CopyInformation(template_nii)``: spacing / origin / direction of the source volume).
    Without a template the depth is ``max(slice) + 1``, float32, identity geometry.
  * ``--task-id T``: files are named ``<output>/T_<id>_pred.nii.gz`` as the trainer names them (:649); otherwise
    ``<output>/<id>/pred.nii.gz``.
  * ``--gt-dir <dir>`` (+ ``--gt-name ce.nii.gz``, ``--mask-name``): the metric pass of inference/get_metric_BraTs.py:54-126
    over the volumes just written — per-id rows + the mean row first — as ``<output>_metric.csv`` (the reference writes the
    same table as .xlsx; its ``mi`` column is ANTs' Mattes MI, not restated: NaN).  ``--metrics-on-device`` (off by default)
    evaluates the table's ``ssim`` column on the rank's GPU (host_io.ssim_torch(device=), metrics.image_metrics);
    ``--metric-table-on-device`` (off by default, needs ``--gt-dir``) evaluates every number column there (nrmse, smape, logac,
    medsymac and psnr through metrics.volume_metrics as well).
Remaining differences from the SimpleITK path: NIfTI headers are copied byte for byte, so the on-disk axis convention is
the template's own (SimpleITK converts LPS <-> RAS when it writes); only single-file NIfTI-1 is handled.

Sampler selection follows TryTrainerDiffusion.on_predict_start (trainers/trainer_use_gaussian_diff.py:586-600):
the diffusion is rebuilt with ``timestep_respacing = str(sample_steps)`` and ``rescale_timesteps = True`` when
sample_steps differs from the training steps, then ``ddim_sample_loop`` or ``p_sample_loop`` is called with
``model_kwargs = dict(c_concat=[images])`` (:602-621).  Multi-GPU: ``--gpus N`` starts one rank per GPU itself (or run
it under torchrun); slices are sharded ``[r::R]``, rank 0's weights are broadcast once, the samples gathered at the end.

Randomness is keyed by SLICE, not by rank or batch position: x_T of slice i comes from a generator seeded with
(seed, i) and the per-step Philox noise of slice i is counter-keyed by i (dsd_set_slice_ids), so a volume gives the same
output on 1 GPU and on N GPUs and with any ``test_batch_size``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import yaml


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model-yaml", required=True)
    ap.add_argument("--infer-yaml", required=True)
    ap.add_argument("--input", required=True, help=".npy [N,C,H,W] condition slices, or a directory <id>/<name>_<slice>.h5")
    ap.add_argument("--input-keys", default="F_Data1", help="h5 input: comma-separated dataset names = condition channels")
    ap.add_argument("--output", required=True)
    ap.add_argument("--ckpt", default=None, help="torch state_dict file (plain tensors; keys may carry model.diffusion_model.)")
    ap.add_argument("--synthetic-weights", type=int, default=None, help="seed: random-init weights (no checkpoint)")
    ap.add_argument("--x-T", default=None, help=".npy [N,1,H,W] start noise (default: torch.randn per batch, as the reference)")
    ap.add_argument("--gpus", type=int, default=1, help="ranks to start (one per GPU) when not already under torchrun")
    ap.add_argument("--template-dir", default=None, help="<dir>/<id>/<template-name>: source volumes whose shape, dtype and header the predictions take")
    ap.add_argument("--template-name", default=None, help="default: <last input key>.nii.gz")
    ap.add_argument("--task-id", default=None, help="name the volumes <output>/<task-id>_<id>_pred.nii.gz (the trainer's naming)")
    ap.add_argument("--gt-dir", default=None, help="<dir>/<id>/<gt-name>: ground truth volumes -> metric table <output>_metric.csv")
    ap.add_argument("--gt-name", default="ce.nii.gz")
    ap.add_argument("--mask-name", default=None, help="optional <gt-dir>/<id>/<mask-name> (> 0 = inside)")
    ap.add_argument("--metrics-on-device", action="store_true",
                    help="the metric table's ssim column (MS-SSIM of every axial slice) on this rank's GPU instead of the host loop")
    ap.add_argument("--metric-table-on-device", action="store_true",
                    help="every number column of the metric table (nrmse, smape, logac, medsymac, ssim, psnr) on this rank's GPU; needs --gt-dir")
    args = ap.parse_args(argv)
    if args.metric_table_on_device and not args.gt_dir:
        ap.error("--metric-table-on-device needs --gt-dir")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_launch(args.gpus, sys.argv[1:] if argv is None else list(argv)))

    from . import parallel
    from ._sched import run_device_loop  # noqa: F401
    from .ldm.util import instantiate_from_config
    from .Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    icfg = yaml.safe_load(open(args.infer_yaml))
    mcfg = yaml.safe_load(open(args.model_yaml))
    mp = mcfg["model"]["params"]
    if world > 1:
        import torch.distributed as dist
        # rehearsal hooks (never set in production; tests/test_infer_gpu.py): DSD_INFER_BACKEND=gloo + DSD_INFER_SINGLE_DEVICE=1 run
        # N ranks over gloo on ONE GPU — the sharding, the bucketed broadcast and the gather on real device memory without N GPUs
        backend = os.environ.get("DSD_INFER_BACKEND", "nccl")
        dev_index = 0 if os.environ.get("DSD_INFER_SINGLE_DEVICE") else local
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
    else:
        dev_index = int(icfg.get("cuda_idx", 0)) if torch.cuda.device_count() > int(icfg.get("cuda_idx", 0)) else 0
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    rank, ws = parallel.world()
    base_seed = int(icfg.get("seed", 2024))
    torch.manual_seed(base_seed)          # the same on every rank: nothing below may depend on the sharding

    uc = dict(mp["unet_config"])
    learn_sigma = bool(mp.get("learn_sigma", False))
    uc["params"] = dict(uc["params"], device_index=dev_index, out_channels=2 if learn_sigma else 1)  # trainer :69
    if rank == 0:
        unet = instantiate_from_config(uc)
    else:
        with parallel.empty_init():            # the values arrive by broadcast: no host initialisation on the other ranks
            unet = instantiate_from_config(uc)
    if rank == 0:
        if args.ckpt:
            sd = torch.load(args.ckpt, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd)
            pre = "model.diffusion_model."
            sd = {(k[len(pre):] if k.startswith(pre) else k): v for k, v in sd.items()}
            unet.load_state_dict({k: v for k, v in sd.items() if k in unet.state_dict()}, strict=True)
        elif args.synthetic_weights is not None:
            g = torch.Generator().manual_seed(args.synthetic_weights)
            with torch.no_grad():
                for p in unet.parameters():
                    if float(p.abs().max()) == 0.0:
                        p.normal_(0.0, 0.02, generator=g)
        else:
            raise SystemExit("give --ckpt or --synthetic-weights")
    if ws > 1:
        # rank 0's weights in 256 MB buckets over RCCL, each uploaded into the library straight from the receive buffer
        # (the analogue of Disc_diff/guided_diffusion/dist_util.py:54-83)
        named = [(nm, tuple(p.shape)) for nm, p in unet.named_parameters()]
        src = dict(unet.named_parameters()) if rank == 0 else None
        parallel.broadcast_params_bucketed(named, (lambda nm: src[nm]) if rank == 0 else None, unet.upload_param, 0, dev)

    ss = icfg["sampler_setting"]
    steps_train = int(mp.get("diffusion_steps", 1000))
    sample_steps = int(ss.get("sample_steps", steps_train))
    respace, rescale = mp.get("timestep_respacing", ""), bool(mp.get("rescale_timesteps", False))
    if sample_steps != steps_train:
        respace, rescale = str(sample_steps), True
    diffusion = create_gaussian_diffusion(steps=steps_train, learn_sigma=learn_sigma,
                                          noise_schedule=mp.get("noise_schedule", "linear"),
                                          predict_xstart=bool(mp.get("predict_xstart", False)), rescale_timesteps=rescale,
                                          timestep_respacing=respace, parameterization=mp.get("parameterization", "eps"))
    which = ss.get("sampler", "ddpm")                       # trainer_use_gaussian_diff.py:597-599
    sample_fn = {"ddim": diffusion.ddim_sample_loop, "dpm": diffusion.dpm_solver_sample_loop}.get(which, diffusion.p_sample_loop)
    extra = {"eta": float(ss.get("ddim_eta", 0))} if which == "ddim" else {}

    h5_paths = None
    if os.path.isdir(args.input):
        from . import host_io
        h5_paths = host_io.find_slice_files(args.input)
        if not h5_paths:
            raise SystemExit(f"no <id>/<name>_<slice>.h5 files under {args.input}")
        n = len(h5_paths)
        mine = parallel.shard_indices(n, rank, ws)
        keys = args.input_keys.split(",")
        # every rank reads ITS slices only (memory O(N / R)); an empty shard still needs the slice shape
        cond_mine = host_io.load_condition_slices([h5_paths[i] for i in mine], keys)
        hw = cond_mine.shape[2:] if len(mine) else host_io.load_condition_slices(h5_paths[:1], keys).shape[2:]
        fetch = lambda pos, idx: cond_mine[pos:pos + len(idx)]
    else:
        cond_all = np.load(args.input, mmap_mode="r")
        n = cond_all.shape[0]
        mine = parallel.shard_indices(n, rank, ws)
        hw = cond_all.shape[2:]
        fetch = lambda pos, idx: cond_all[idx]
    xT_all = np.load(args.x_T, mmap_mode="r") if args.x_T else None
    bs = int(icfg.get("test_batch_size", 16))
    outs = []
    seeded = {} if which == "dpm" else {"seed": base_seed}   # DPM-Solver++ is deterministic after x_T
    for i in range(0, len(mine), bs):
        idx = mine[i:i + bs]
        images = torch.from_numpy(np.ascontiguousarray(fetch(i, idx))).float().to(dev)
        B, _, H, W = images.shape
        if xT_all is not None:
            noise = torch.from_numpy(np.ascontiguousarray(xT_all[idx])).float().to(dev)
        else:
            noise = torch.stack([slice_noise(base_seed, j, (1, H, W)) for j in idx]).to(dev)
        unet.set_slice_ids(idx)
        outs.append(sample_fn(unet, (B, 1, H, W), noise=noise, clip_denoised=bool(mp.get("clip_denoised", True)),
                              model_kwargs=dict(c_concat=[images]), **extra, **seeded))
    unet.set_slice_ids(None)
    local_out = torch.cat(outs) if outs else torch.zeros((0, 1) + tuple(hw), device=dev)
    full = parallel.gather_slices(local_out, n, 0)
    if rank == 0 and h5_paths is not None and not args.output.endswith(".npy"):
        from . import host_io
        asm = host_io.VolumeAssembler()
        asm.add_paths(h5_paths, full.cpu().numpy())
        tname = args.template_name or (args.input_keys.split(",")[-1] + ".nii.gz")
        written = {}
        for id_ in asm.ids():
            template, thdr = (None, None)
            if args.template_dir:
                template, thdr = host_io.read_nifti(os.path.join(args.template_dir, id_, tname))
            vol = asm.volume(id_, template=template)
            if args.task_id is not None:
                os.makedirs(args.output, exist_ok=True)
                path = os.path.join(args.output, f"{args.task_id}_{id_}_pred.nii.gz")
            else:
                os.makedirs(os.path.join(args.output, id_), exist_ok=True)
                path = os.path.join(args.output, id_, "pred.nii.gz")
            host_io.write_nifti(path, vol, template_header=thdr)
            written[id_] = path
            print(f"wrote {path}: {tuple(vol.shape)} {vol.dtype}")
        if args.gt_dir:
            table = host_io.metric_table(written, args.gt_dir, args.gt_name, args.mask_name,
                                         device=dev if args.metrics_on_device or args.metric_table_on_device else None,
                                         table_on_device=args.metric_table_on_device)
            csv_path = args.output.rstrip("/") + "_metric.csv"
            host_io.write_metric_csv(csv_path, table)
            print(f"wrote {csv_path}: {len(table) - 1} ids + mean row")
    elif rank == 0:
        np.save(args.output, full.cpu().numpy())
        print(f"wrote {args.output}: {tuple(full.shape)}")
    if ws > 1:
        torch.distributed.destroy_process_group()


def slice_noise(seed: int, slice_index: int, shape):
    """x_T of one slice: N(0,1) from a generator keyed by (seed, global slice index) — independent of rank and batch."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(slice_index)) % (2 ** 63 - 1))
    return torch.randn(shape, generator=g)


def _launch(n, argv):
    """--gpus N outside torchrun: start N ranks of this module (one per GPU); this process never touches the GPU."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m",
                            "diffusion_models_dsdiff_amd.infer_2d"] + list(argv), env=env)


if __name__ == "__main__":
    main()
