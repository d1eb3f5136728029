"""CPU restatement (torch, fp32) of the DPM-Solver variants beyond oracle/dpm.py's multistep order <= 2, shared by
test_dpm_family_cpu.py and test_dpm_family_gpu.py.  Written from the reference, Disc_diff/guided_diffusion/sampler.py:
get_orders_and_timesteps_for_singlestep_solver :445-501, dpm_solver_first_update :509-553, singlestep second / third update
:555-635 / :637-758, multistep second / third update :760-816 / :818-868, sample :1121-1213, inverse :1001-1015; the noise
schedule, the time grids and dynamic thresholding come from oracle/dpm.py.  Scalars are (1,)-tensors as in a CPU run of the
reference, so every product below rounds where the reference's does.

``ref_sample`` is the reference's loop.  ``eval_cpu`` is one row of a product DpmProgram in the same torch operations the HIP
kernels perform (sampler.hip dpm_model_kernel / dpm_eval_kernel): the bit-exact reference of the per-evaluation op."""
import torch

from oracle import dpm as ODPM


def singlestep_orders(ns, steps, order, skip_type, t_T, t_0):
    """:445-501."""
    if order == 3:
        K = steps // 3 + 1
        orders = [3] * (K - 2) + [2, 1] if steps % 3 == 0 else ([3] * (K - 1) + [1] if steps % 3 == 1 else [3] * (K - 1) + [2])
    elif order == 2:
        K = steps // 2 if steps % 2 == 0 else steps // 2 + 1
        orders = [2] * K if steps % 2 == 0 else [2] * (K - 1) + [1]
    else:
        K, orders = 1, [1] * steps
    if skip_type == "logSNR":
        return ODPM.time_steps(ns, skip_type, t_T, t_0, K), orders
    return ODPM.time_steps(ns, skip_type, t_T, t_0, steps)[torch.cumsum(torch.tensor([0] + orders), 0)], orders


@torch.no_grad()
def ref_sample(net, ns, x, *, steps, order=2, skip_type="time_uniform", method="multistep", model_type="noise",
               algorithm="dpmsolver++", thresholding=False, lower_order_final=True, denoise_to_zero=False, solver_type="dpmsolver",
               t_start=None, t_end=None, inverse=False, return_intermediate=False, net_uncond=None, scale=1., ratio=0.995,
               max_val=1., record=None):
    """DPM_Solver.sample / .inverse.  net(x, t_input [B]) -> the network output on the state (condition closed over);
    ``net_uncond``: the same under the unconditional condition — classifier-free guidance on the two noise predictions
    (dpm_solver_pytorch.py:324-332).  ``record``: a dict that receives t / alpha / sigma of every evaluation and (r1, r2) of
    every singlestep step."""
    pp, B = algorithm == "dpmsolver++", x.shape[0]
    if inverse:
        t_0 = 1. / ns.total_N if t_start is None else t_start
        t_T = ns.T if t_end is None else t_end
        t_T, t_0 = t_0, t_T                                   # sample(t_start=t_0, t_end=t_T)
    else:
        t_0 = 1. / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
    if record is not None:
        record.update(t=[], alpha=[], sigma=[], r=[])

    def noise_pred(f, x, t):                                  # model_wrapper.noise_pred_fn :247-265
        tc = t.expand(B)
        out = f(x, (tc - 1. / ns.total_N) * 1000.)[:, :x.shape[1]]
        if model_type == "noise":
            return out
        a, s = ns.alpha(tc)[:, None, None, None], ns.std(tc)[:, None, None, None]
        return (x - a * out) / s if model_type == "x_start" else a * out + s * x

    def model_fn(x, t, data=pp):                              # :390-414
        t = t.reshape(-1)
        if record is not None:
            record["t"].append(float(t)), record["alpha"].append(float(ns.alpha(t))), record["sigma"].append(float(ns.std(t)))
        eps = noise_pred(net, x, t)
        if net_uncond is not None:
            eu = noise_pred(net_uncond, x, t)
            eps = eu + scale * (eps - eu)
        if not data:
            return eps
        x0 = (x - ns.std(t) * eps) / ns.alpha(t)
        return ODPM.dynamic_threshold(x0, ratio, max_val) if thresholding else x0

    def scal(s, t):
        s, t = s.reshape(-1), t.reshape(-1)
        h = ns.lam(t) - ns.lam(s)
        if pp:
            return h, ns.std(t) / ns.std(s), torch.exp(ns.log_mean(t)), torch.expm1(-h)
        return h, torch.exp(ns.log_mean(t) - ns.log_mean(s)), ns.std(t), torch.expm1(h)

    def first(x, s, t, m):                                    # :509-553
        h, cx, lead, phi_1 = scal(s, t)
        return cx * x - (lead * phi_1) * m

    def ms_second(x, ms, ts, t):                              # :760-816
        m1, m0 = ms[-2], ms[-1]
        h, cx, lead, phi_1 = scal(ts[-1], t)
        r0 = (ns.lam(ts[-1].reshape(-1)) - ns.lam(ts[-2].reshape(-1))) / h
        D1_0 = (1. / r0) * (m0 - m1)
        if solver_type == "dpmsolver":
            return cx * x - (lead * phi_1) * m0 - 0.5 * (lead * phi_1) * D1_0
        if pp:
            return cx * x - (lead * phi_1) * m0 + (lead * (phi_1 / h + 1.)) * D1_0
        return cx * x - (lead * phi_1) * m0 - (lead * (phi_1 / h - 1.)) * D1_0

    def ms_third(x, ms, ts, t):                               # :818-868
        m2, m1, m0 = ms
        l2, l1, l0 = (ns.lam(v.reshape(-1)) for v in ts)
        h, cx, lead, phi_1 = scal(ts[-1], t)
        r0, r1 = (l0 - l1) / h, (l1 - l2) / h
        D1_0 = (1. / r0) * (m0 - m1)
        D1_1 = (1. / r1) * (m1 - m2)
        D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
        D2 = (1. / (r0 + r1)) * (D1_0 - D1_1)
        if pp:
            phi_2 = phi_1 / h + 1.
            phi_3 = phi_2 / h - 0.5
            return cx * x - (lead * phi_1) * m0 + (lead * phi_2) * D1 - (lead * phi_3) * D2
        phi_2 = phi_1 / h - 1.
        phi_3 = phi_2 / h - 0.5
        return cx * x - (lead * phi_1) * m0 - (lead * phi_2) * D1 - (lead * phi_3) * D2

    def ss_second(x, s, t, r1):                               # :555-635
        h, cx, lead, phi_1 = scal(s, t)
        s1 = ns.inv_lam(ns.lam(s.reshape(-1)) + r1 * h)
        _, cx1, lead1, _ = scal(s, s1)
        phi_11 = torch.expm1(-r1 * h) if pp else torch.expm1(r1 * h)
        m_s = model_fn(x, s)
        m_s1 = model_fn(cx1 * x - (lead1 * phi_11) * m_s, s1)
        if solver_type == "dpmsolver":
            return cx * x - (lead * phi_1) * m_s - (0.5 / r1) * (lead * phi_1) * (m_s1 - m_s)
        if pp:
            return cx * x - (lead * phi_1) * m_s + (1. / r1) * (lead * (phi_1 / h + 1.)) * (m_s1 - m_s)
        return cx * x - (lead * phi_1) * m_s - (1. / r1) * (lead * (phi_1 / h - 1.)) * (m_s1 - m_s)

    def ss_third(x, s, t, r1, r2):                            # :637-758
        h, cx, lead, phi_1 = scal(s, t)
        s1, s2 = ns.inv_lam(ns.lam(s.reshape(-1)) + r1 * h), ns.inv_lam(ns.lam(s.reshape(-1)) + r2 * h)
        _, cx1, lead1, _ = scal(s, s1)
        _, cx2, lead2, _ = scal(s, s2)
        if pp:
            phi_11, phi_12 = torch.expm1(-r1 * h), torch.expm1(-r2 * h)
            phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
            phi_2 = phi_1 / h + 1.
        else:
            phi_11, phi_12 = torch.expm1(r1 * h), torch.expm1(r2 * h)
            phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
            phi_2 = phi_1 / h - 1.
        phi_3 = phi_2 / h - 0.5
        m_s = model_fn(x, s)
        m_s1 = model_fn(cx1 * x - (lead1 * phi_11) * m_s, s1)
        if pp:
            x_s2 = cx2 * x - (lead2 * phi_12) * m_s + r2 / r1 * (lead2 * phi_22) * (m_s1 - m_s)
        else:
            x_s2 = cx2 * x - (lead2 * phi_12) * m_s - r2 / r1 * (lead2 * phi_22) * (m_s1 - m_s)
        m_s2 = model_fn(x_s2, s2)
        if solver_type == "dpmsolver":
            if pp:
                return cx * x - (lead * phi_1) * m_s + (1. / r2) * (lead * phi_2) * (m_s2 - m_s)
            return cx * x - (lead * phi_1) * m_s - (1. / r2) * (lead * phi_2) * (m_s2 - m_s)
        D1_0 = (1. / r1) * (m_s1 - m_s)
        D1_1 = (1. / r2) * (m_s2 - m_s)
        D1 = (r2 * D1_0 - r1 * D1_1) / (r2 - r1)
        D2 = 2. * (D1_1 - D1_0) / (r2 - r1)
        if pp:
            return cx * x - (lead * phi_1) * m_s + (lead * phi_2) * D1 - (lead * phi_3) * D2
        return cx * x - (lead * phi_1) * m_s - (lead * phi_2) * D1 - (lead * phi_3) * D2

    inter = []
    if method == "multistep":                                 # :1136-1180
        ts = ODPM.time_steps(ns, skip_type, t_T, t_0, steps)
        t_prev, m_prev = [ts[0]], [model_fn(x, ts[0])]
        inter.append(x)

        def update(x, t, so):
            if so == 1:
                return first(x, t_prev[-1], t, m_prev[-1])
            return ms_second(x, m_prev, t_prev, t) if so == 2 else ms_third(x, m_prev, t_prev, t)
        for step in range(1, order):
            x = update(x, ts[step], step)
            inter.append(x)
            t_prev.append(ts[step])
            m_prev.append(model_fn(x, ts[step]))
        for step in range(order, steps + 1):
            so = min(order, steps + 1 - step) if (lower_order_final and steps < 10) else order
            x = update(x, ts[step], so)
            inter.append(x)
            for i in range(order - 1):
                t_prev[i], m_prev[i] = t_prev[i + 1], m_prev[i + 1]
            t_prev[-1] = ts[step]
            if step < steps:
                m_prev[-1] = model_fn(x, ts[step])
    else:                                                     # :1181-1204
        if method == "singlestep":
            outer, orders = singlestep_orders(ns, steps, order, skip_type, t_T, t_0)
        else:
            K = steps // order
            outer, orders = ODPM.time_steps(ns, skip_type, t_T, t_0, K), [order] * K
        for step, so in enumerate(orders):
            s, t = outer[step], outer[step + 1]
            lam_in = ns.lam(ODPM.time_steps(ns, skip_type, s.item(), t.item(), so))
            h_in = lam_in[-1] - lam_in[0]
            r1 = None if so <= 1 else (lam_in[1] - lam_in[0]) / h_in
            r2 = None if so <= 2 else (lam_in[2] - lam_in[0]) / h_in
            if record is not None:
                record["r"].append([float(r1) if r1 is not None else 0., float(r2) if r2 is not None else 0.])
            if so == 1:
                x = first(x, s, t, model_fn(x, s))
            else:
                x = ss_second(x, s, t, r1) if so == 2 else ss_third(x, s, t, r1, r2)
            inter.append(x)
    if denoise_to_zero:                                       # :1207-1213
        x = model_fn(x, torch.ones((1,)) * t_0, data=True)
        inter.append(x)
    return (x, inter) if return_intermediate else x


READS = (1, 1, 2, 3, 1, 2, 2, 2, 3)                           # history planes a kind reads (include/dsdiff.h DSD_DPM_*)


def eval_cpu(prog, k, out, x, hist, base, out_u=None, scale=1.):
    """Evaluation k of a product DpmProgram after the network: the operations of dpm_model_kernel, the thresholding and
    dpm_eval_kernel, one fp32 torch op each.  out [B,Cm*C,H,W] (the first C channels are read), x [B,C,H,W] the state the
    network read; hist (list of three planes) and base (a list holding one tensor) are updated; returns the next state."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    kind, pred = int(prog.kind[k]), int(prog.c.pred)
    alpha, sigma = f(prog.alpha[k]), f(prog.sigma[k])
    c = [f(v) for v in prog.coef[k]]
    w, a, b, cc = (int(v) for v in prog.slot[k])
    C = x.shape[1]

    def noise(o):
        o = o[:, :C]
        return o if pred == 0 else ((x - alpha * o) / sigma if pred == 1 else alpha * o + sigma * x)
    eps = noise(out)
    if out_u is not None:
        eu = noise(out_u)
        eps = eu + f(scale) * (eps - eu)
    data = bool(prog.c.data_pred) or kind == 0
    m = (x - sigma * eps) / alpha if data else eps
    if prog.c.thresholding and data:
        m = ODPM.dynamic_threshold(m, float(prog.c.threshold_ratio), float(prog.c.threshold_max))
    hist[w] = m
    ma, mb, mc = hist[a], hist[b] if READS[kind] >= 2 else None, hist[cc] if READS[kind] >= 3 else None
    if kind == 4:
        base[0] = x
    xb = base[0] if kind >= 5 else x
    if kind == 0:
        return ma
    lin = c[0] * xb - c[1] * ma
    if kind in (1, 4):
        return lin
    if kind == 2:
        return lin - c[2] * (c[3] * (ma - mb))
    if kind == 3:
        d10, d11 = c[4] * (ma - mb), c[5] * (mb - mc)
        dd = d10 - d11
        return (lin + c[2] * (d10 + c[6] * dd)) - c[3] * (c[7] * dd)
    if kind in (5, 6, 7):
        return lin - c[2] * (mb - ma)
    d10, d11 = c[4] * (mb - ma), c[5] * (mc - ma)
    d1 = (c[7] * d10 - c[6] * d11) / c[8]
    d2 = 2. * (d11 - d10) / c[8]
    return (lin + c[2] * d1) - c[3] * d2


@torch.no_grad()
def run_program_cpu(prog, net, x, net_uncond=None, scale=1.):
    """A product DpmProgram interpreted on the CPU; returns (sample, kept states)."""
    hist, base, kept = [None] * 3, [None], []
    for k in range(prog.steps):
        t = torch.full((x.shape[0],), float(prog.t_input[k]))
        x = eval_cpu(prog, k, net(x, t), x, hist, base, net_uncond(x, t) if net_uncond is not None else None, scale)
        if prog.keep[k]:
            kept.append(x)
    return x, kept
