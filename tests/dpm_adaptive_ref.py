"""CPU restatement (torch, fp32) of the adaptive step-size DPM-Solver, shared by test_dpm_adaptive_cpu.py and
test_dpm_adaptive_gpu.py.  Written from the reference, Disc_diff/guided_diffusion/sampler.py:921-980: the loop on (1,)-tensors
(the step size, the accept / reject decision, the end test) with the noise schedule of oracle/dpm.py; a trial takes its
coefficient rows from the product (DPM_Solver.adaptive_trial_program, i.e. _singlestep_evals) and runs them through
dpm_family_ref.eval_cpu — the torch operations of the HIP kernels — so a run that equals the reference's pins the rows, the
lower-order row and the step-size arithmetic.

``lower_cpu`` / ``error_cpu`` are the operations of dpm_adaptive_error_kernel, one fp32 torch op each (the bit-exact reference of
x_lower); ``error_f64`` is the error norm in float64 on the same inputs."""
import torch

import dpm_family_ref as R


def lower_cpu(lower, order, base, ma, mb):
    """x_lower of a trial of ``order`` from the planes the step left: c0*x_s - c1*model_s [- c2*(model_s1 - model_s)]."""
    c = [torch.tensor(float(v), dtype=torch.float32) for v in lower]
    lin = c[0] * base - c[1] * ma
    return lin if order == 2 else lin - c[2] * (mb - ma)


def error_cpu(x_higher, x_lower, x_prev, atol, rtol):
    """:969-971 per sample (the reference then takes .max() over the batch)."""
    delta = torch.max(torch.ones_like(x_lower) * atol, rtol * torch.max(torch.abs(x_lower), torch.abs(x_prev)))
    v = (x_higher - x_lower) / delta
    return torch.sqrt(torch.square(v.reshape((v.shape[0], -1))).mean(dim=-1))


def error_f64(x_higher, x_lower, x_prev, atol, rtol):
    """The same norm in float64 from the fp32 inputs; atol / rtol as the fp32 values the kernel receives."""
    a, r = (float(torch.tensor(v, dtype=torch.float32)) for v in (atol, rtol))
    xh, xl, xp = x_higher.double(), x_lower.double(), x_prev.double()
    delta = torch.clamp(r * torch.max(xl.abs(), xp.abs()), min=a)
    v = (xh - xl) / delta
    return torch.sqrt(v.reshape(v.shape[0], -1).pow(2).mean(dim=-1))


@torch.no_grad()
def trial_cpu(prog, lower, order, net, x, x_prev, atol, rtol, net_uncond=None, scale=1.):
    """One trial interpreted on the CPU: (x_higher, x_lower, E [B])."""
    hist, base = [None] * 3, [None]
    xs = x
    for k in range(prog.steps):
        t = torch.full((x.shape[0],), float(prog.t_input[k]))
        x = R.eval_cpu(prog, k, net(x, t), x, hist, base, net_uncond(x, t) if net_uncond is not None else None, scale)
    assert base[0] is xs
    x_lower = lower_cpu(lower, order, base[0], hist[int(prog.slot[0, 0])], hist[int(prog.slot[1, 0])])
    return x, x_lower, error_cpu(x, x_lower, x_prev, atol, rtol)


@torch.no_grad()
def run_adaptive_cpu(sol, ns, net, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5,
                     solver_type="dpmsolver", net_uncond=None, scale=1., trial=None):
    """dpm_solver_adaptive :942-980.  ``sol``: the product's DPM_Solver (rows only); ``ns``: oracle/dpm.py's NoiseSchedule.
    ``trial(prog, lower, x, x_prev) -> (x_higher, x_lower, E [B] on the CPU)`` replaces the CPU trial (the GPU tests' per-step
    path).  Returns (sample, trace [(s, t, h, E, accepted)], nfe)."""
    s = t_T * torch.ones((1,))
    lambda_s = ns.lam(s)
    lambda_0 = ns.lam(t_0 * torch.ones_like(s))
    h = h_init * torch.ones_like(s)
    x_prev, nfe, trace = x, 0, []
    while torch.abs((s - t_0)).mean() > t_err:
        t = ns.inv_lam(lambda_s + h)
        prog, lower = sol.adaptive_trial_program(s, t, order, solver_type)
        if trial is not None:
            x_higher, x_lower, E_b = trial(prog, lower, x, x_prev)
        else:
            x_higher, x_lower, E_b = trial_cpu(prog, lower, order, net, x, x_prev, atol, rtol, net_uncond, scale)
        E = E_b.max()
        accepted = bool(torch.all(E <= 1.))
        trace.append((float(s), float(t), float(h), float(E), accepted))
        if accepted:
            x, s, x_prev = x_higher, t, x_lower
            lambda_s = ns.lam(s)
        h = torch.min(theta * h * torch.float_power(E, -1. / order).float(), lambda_0 - lambda_s)
        nfe += order
    return x, trace, nfe
