"""create_gaussian_diffusion — drop-in for training_project/utils/script_util.py:129-169
(same function in Disc_diff/guided_diffusion/script_util.py) — and that file's sr_create_model /
sr_create_model_and_diffusion (:52-126), the builders of the four-stream DisC-Diff denoiser."""
from . import gaussian_diffusion as gd
from .respace import SpacedDiffusion, space_timesteps


def sr_create_model_and_diffusion(args):
    """:52-87.  ``args``: a namespace with the reference's command-line fields."""
    model = sr_create_model(
        args.image_size, args.in_channel, args.num_channels, args.num_res_blocks, learn_sigma=args.learn_sigma,
        use_checkpoint=args.use_checkpoint, attention_resolutions=args.attention_resolutions, num_heads=args.num_heads,
        num_head_channels=args.num_head_channels, num_heads_upsample=args.num_heads_upsample,
        use_scale_shift_norm=args.use_scale_shift_norm, dropout=args.dropout, resblock_updown=args.resblock_updown,
        use_fp16=args.use_fp16)
    diffusion = create_gaussian_diffusion(
        steps=args.diffusion_steps, learn_sigma=args.learn_sigma, noise_schedule=args.noise_schedule, use_kl=args.use_kl,
        predict_xstart=args.predict_xstart, rescale_timesteps=args.rescale_timesteps,
        rescale_learned_sigmas=args.rescale_learned_sigmas, timestep_respacing=args.timestep_respacing,
        parameterization=args.parameterization)
    return model, diffusion


def sr_create_model(image_size, in_channel, num_channels, num_res_blocks, learn_sigma, use_checkpoint, attention_resolutions,
                    num_heads, num_head_channels, num_heads_upsample, use_scale_shift_norm, dropout, resblock_updown, use_fp16,
                    device_index=0):
    """:90-126: channel_mult (1, 1, 2, 2, 3, 3), attention at 8 / 16 / 32 whatever ``attention_resolutions`` says, out_channels
    doubled under learn_sigma.  ``device_index`` is an extension (negative: parameter table only)."""
    from .unet import SuperResModelNew
    channel_mult = (1, 1, 2, 2, 3, 3)
    attention_ds = [8, 16, 32]
    return SuperResModelNew(
        image_size=image_size, in_channels=in_channel, model_channels=num_channels,
        out_channels=(in_channel if not learn_sigma else in_channel * 2), num_res_blocks=num_res_blocks,
        attention_resolutions=tuple(attention_ds), dropout=dropout, channel_mult=channel_mult, use_checkpoint=use_checkpoint,
        num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
        use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown, use_fp16=use_fp16, device_index=device_index)


def create_gaussian_diffusion(*, steps=1000, learn_sigma=False, sigma_small=False, noise_schedule="linear",
                              use_kl=False, predict_xstart=False, rescale_timesteps=False,
                              rescale_learned_sigmas=False, timestep_respacing="", parameterization="eps"):
    betas = gd.get_named_beta_schedule(noise_schedule, steps)
    if use_kl:
        loss_type = gd.LossType.RESCALED_KL
    elif rescale_learned_sigmas:
        loss_type = gd.LossType.RESCALED_MSE
    else:
        loss_type = gd.LossType.MSE
    if not timestep_respacing:
        timestep_respacing = [steps]
    if learn_sigma:
        var_type = gd.ModelVarType.LEARNED_RANGE
    else:
        var_type = gd.ModelVarType.FIXED_SMALL if sigma_small else gd.ModelVarType.FIXED_LARGE
    return SpacedDiffusion(
        use_timesteps=space_timesteps(steps, timestep_respacing),
        betas=betas,
        model_mean_type=gd.ModelMeanType.START_X if predict_xstart else gd.ModelMeanType.EPSILON,
        model_var_type=var_type,
        loss_type=loss_type,
        rescale_timesteps=rescale_timesteps,
        parameterization=parameterization,
    )
