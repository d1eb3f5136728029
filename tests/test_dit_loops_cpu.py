"""The DiT as a denoiser of the device sampling loops — what can be checked without a GPU: the channel bookkeeping helper, the
fp32 operation order of the multi-channel learned-range update, the stubs' refusals, and the conditioning of the oracle chains
tests/test_dit_loops_gpu.py holds the device loops to.

PINNED BY THE REFERENCE: the network of every chain is oracle/dit.py, equal to the last bit to the reference's own DiT on the
fixtures of tests/golden/dit.npz (tests/test_pinned_cpu.py), which rest on the reference's code and on the three timm modules
of tests/golden/ref_standins.py (timm is absent from the image; witnessed against nn.MultiheadAttention and F.unfold); the
sampler arithmetic is pinned by oracle/samplers.py as everywhere else.  Still unpinned: the half-precision modes' rounding
places and host_io.py's metrics."""
import numpy as np
import pytest
import torch

import dit_loops_util as U
from oracle import samplers as OS
from util import rel_l2


def test_channel_helper_layouts_and_misfits():
    from diffusion_models_dsdiff_amd._sched import dit_state_channels
    assert dit_state_channels(4, True, 3) == (1, 2)          # the shipped yaml: 1 state + 3 condition channels, learned sigma
    assert dit_state_channels(6, True, 4) == (2, 4)
    assert dit_state_channels(3, False, 0) == (3, 3)         # unconditional
    assert dit_state_channels(5, True, 4) == (1, 2)          # in_channels // 3 * 2 (sic)
    for name, (kw, Cz, Cc) in U.MODELS.items():
        assert dit_state_channels(kw["in_channels"], kw.get("learn_sigma", True), Cc)[0] == Cz, name
    with pytest.raises(ValueError, match=r"4 input channels.*2 output channels.*1 conditioning.*state has 3"):
        dit_state_channels(4, True, 1)                       # 3 state channels against 2 output channels
    with pytest.raises(ValueError, match=r"6 input channels.*4 output channels.*0 conditioning.*state has 6"):
        dit_state_channels(6, True, 0)
    with pytest.raises(ValueError, match=r"4 input channels.*4 output channels.*3 conditioning.*state has 1"):
        dit_state_channels(4, False, 3)                      # without learn_sigma the output is as wide as the input
    with pytest.raises(ValueError, match="leaves no state beside 4"):
        dit_state_channels(4, True, 4)
    with pytest.raises(ValueError, match="leaves no state"):
        dit_state_channels(4, True, -1)


def test_find_unet_takes_no_stub_for_a_dit():
    """Nothing but the native classes is a denoiser of the device loops: stubs keep getting None, and the loops' prologue its
    'no native denoiser'."""
    from diffusion_models_dsdiff_amd import _sched

    class Stub(torch.nn.Module):
        in_channels, learn_sigma, input_size = 4, True, 16

        def forward(self, x, t, y=None, cond=None):
            return x

    class Wrapper(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.diffusion_model = Stub()

    class Outer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model = Wrapper()

    for m in (Stub(), Wrapper(), Outer(), lambda x, t: x):
        assert _sched.find_unet(m) is None
    x, c = torch.zeros(2, 1, 16, 16), torch.zeros(2, 3, 16, 16)
    sched = _sched.Schedule(0, 0, np.zeros((2, 8), np.float32), np.zeros(2, np.float32), np.ones(2, np.int32))
    with pytest.raises(RuntimeError, match="no native denoiser"):
        _sched.run_device_loop(_sched.find_unet(Wrapper()), sched, x, c)
    with pytest.raises(RuntimeError, match="no native denoiser"):
        _sched.run_plms_loop(_sched.find_unet(Outer()), sched, x, c)
    with pytest.raises(RuntimeError, match="no native denoiser"):
        _sched.run_invert_loop(_sched.find_unet(Stub()), np.zeros((2, 2), np.float32), x, c)


def test_multichannel_learned_range_rows_reproduce_the_oracle_loop():
    """The coefficient rows handed to dsd_sample, replayed on the CPU in the update kernel's fp32 operation order
    (sampler.hip sampler_update_value, emulated with torch fp32 ops), must reproduce the oracle's p_sample_loop on an analytic
    network of two state channels whose output carries a variance half: this pins the split by Cz, the pairing of channel c with
    variance channel Cz + c and frac*max_log + (1 - frac)*min_log without a GPU."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    Cz, B, H = 2, 3, 6

    def net(x, t):          # [B,2,H,H] -> [B,4,H,H]: the two halves mix both state channels differently
        s = torch.sin(t.float() / 1000.)[:, None, None, None]
        mean = 0.3 * x + s + 0.05 * x.flip(1).flip(-1)
        var = torch.tanh(0.7 * x.flip(1) - s + torch.tensor([0.2, -0.4])[None, :, None, None])
        return torch.cat([mean, var], 1)
    for kw in (dict(steps=1000, timestep_respacing="10", learn_sigma=True, rescale_timesteps=True),
               dict(steps=100, timestep_respacing="", learn_sigma=True, noise_schedule="cosine")):
        d = create_gaussian_diffusion(**kw)
        sc = d._schedule(False, 0.0, True)
        assert sc.c.learned_range and sc.steps == d.num_timesteps
        x_T, z = U.randn((B, Cz, H, H), 31), U.randn((sc.steps, B, Cz, H, H), 32)
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        x = x_T.clone()
        for k in range(sc.steps):
            c = [f(v) for v in sc.coef[k]]
            out = net(x, torch.full((B,), float(sc.t_model[k])))
            eps, var = out[:, :Cz], out[:, Cz:]
            x0 = (c[2] * x - c[3] * eps).clamp(-1, 1)
            mean = c[4] * x0 + c[5] * x
            frac = (var + 1.) / 2.
            logvar = frac * c[7] + (1. - frac) * c[6]
            nz = 1. if sc.nonzero[k] else 0.
            x = mean + nz * torch.exp(0.5 * logvar) * z[k]
        want = OS.DiffusionA(**kw).p_sample_loop(net, x_T, z)
        np.testing.assert_array_equal(x.numpy(), want.numpy())


@pytest.mark.parametrize("name", sorted(U.CHAIN_BATCH))
@pytest.mark.parametrize("kind", U.CHAINS)
def test_oracle_chains_are_well_conditioned(name, kind):
    """The guard of the GPU-against-oracle chains (as tests/golden/gen_plms.py): Gaussian noise of 3e-6 relative RMS on every
    network output — the size of the GPU-against-oracle forward error — must move the chain's result by less than 2e-5, a fifth
    of the 1e-4 chain bar, or the bar would measure the chain's conditioning rather than the loop."""
    y = U.oracle_chain_cached(name, kind)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 1e-2
    move = rel_l2(U.oracle_chain(name, kind, perturb=True), y)
    print(f"{name} {kind}: max |y| {float(y.abs().max()):.3f}, moved {move:.2e} by {U.PERTURB:g} noise on the network output")
    assert move < U.MOVE_MAX


def test_a_dit_with_labels_or_its_own_cond_keeps_the_per_step_path():
    """The device loops hand a DiT its input and t only.  A call whose model_kwargs carry anything else (labels ``y``,
    DiT.forward's own ``cond``) must keep the per-step path, where the network receives them; with at most ``c_concat`` the DiT
    is the loops' denoiser, bare or wrapped.  The class check is all find_unet looks at, so an unbuilt instance stands in for a
    handle (building one needs the GPU)."""
    from types import SimpleNamespace
    from diffusion_models_dsdiff_amd import _sched
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion, sampler
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.model import DSUnetModel
    dit = DiT.__new__(DiT)
    wrapped = SimpleNamespace(diffusion_model=dit)
    outer = SimpleNamespace(model=wrapped)
    c, y = torch.zeros(2, 3, 16, 16), torch.tensor([1, 2])
    for m in (dit, wrapped, outer):
        assert _sched.find_unet(m) is dit
        assert _sched.loop_denoiser(m) is dit and _sched.loop_denoiser(m, {}) is dit
        assert _sched.loop_denoiser(m, dict(c_concat=[c])) is dit
        assert _sched.loop_denoiser(m, dict(y=y)) is None
        assert _sched.loop_denoiser(m, dict(cond=c)) is None
        assert _sched.loop_denoiser(m, dict(c_concat=[c], y=y)) is None
    unet = DSUnetModel.__new__(DSUnetModel)                  # the U-Nets' routing is what it was: model_kwargs do not matter
    assert _sched.loop_denoiser(unet, dict(c_concat=[c], y=y)) is unet
    assert _sched.loop_denoiser(lambda x, t: x, dict(c_concat=[c])) is None
    assert gaussian_diffusion.loop_denoiser is _sched.loop_denoiser and sampler.loop_denoiser is _sched.loop_denoiser

    # the shims act on it: with labels the network itself is called, once per step, with the labels
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    seen = []

    class Recording(DiT):
        def forward(self, x, t, y=None, cond=None):
            seen.append((y, cond))
            raise _Reached()

    class _Reached(Exception):
        pass
    rec = Recording.__new__(Recording)
    torch.nn.Module.__init__(rec)                            # callable as a module, still without a handle
    d = create_gaussian_diffusion(steps=1000, timestep_respacing="4", learn_sigma=True)
    for kw in (dict(y=y), dict(cond=c)):
        with pytest.raises(_Reached):
            d.p_sample_loop(rec, (2, 1, 16, 16), noise=torch.zeros(2, 1, 16, 16), model_kwargs=kw, device="cpu")
    assert seen[0][0] is y and seen[1][1] is c
    ns = sampler.NoiseScheduleVP(schedule="discrete", betas=U.spaced_betas())
    sol = sampler.DPM_Solver(sampler.model_wrapper(rec, ns, model_kwargs=dict(y=y)), ns, algorithm_type="dpmsolver++")
    with pytest.raises((_Reached, RuntimeError)) as ei:
        sol.sample(torch.zeros(2, 1, 16, 16), steps=4, order=2, skip_type="logSNR")
    assert ei.type is _Reached or "MI355X only" in str(ei.value)     # the CPU refusal sits in front of the per-step loop
