"""Restatements for the self-conditioning tests (tests/test_host_selfcond.py, tests/test_gpu_selfcond.py): the estimate x0~ of
vdx_selfcond_x0 in fp32 (the kernel's roundings, one per operation: torch on the CPU fuses nothing) and in fp64, and one self-conditioned
step from public pieces.  Nothing here needs a GPU or libvdx.  A plain module: nothing here is collected."""
import torch


def to_channel_first(eps_cl):
    """Channel-last [B,F,H,W,C] -> [B,C,F,H,W], contiguous."""
    return eps_cl.permute(0, 4, 1, 2, 3).contiguous()


def x0_estimate(x, eps_cl, t, tables, *, clip=True, thres=None, dtype=torch.float32):
    """x0~ [B,C,F,H,W] of x [B,C,F,H,W] and the channel-last eps_hat [B,F,H,W,C] at levels t [B] (clamped to [0, T - 1]) with rows 0, 1
    of the [5][T] step tables: fl(k_recip x) - fl(k_recipm1 eps), then with clip min(max(., -s), s) / s, s = thres[b] or 1.  dtype
    float32: the kernel's bits; float64: the same expression on the widened inputs."""
    T = tables.shape[1]
    tb = t.long().clamp(0, T - 1)
    shape = (-1, 1, 1, 1, 1)
    kr, km = tables[0][tb].to(dtype).reshape(shape), tables[1][tb].to(dtype).reshape(shape)
    x0 = kr * x.to(dtype) - km * to_channel_first(eps_cl).to(dtype)
    if clip:
        s = torch.ones(x.shape[0], dtype=dtype) if thres is None else thres.to(dtype)
        s = s.reshape(shape)
        x0 = torch.minimum(torch.maximum(x0, -s), s) / s
    return x0


def self_cond_step(net, x, est, t, tables, *, to_eps=None, thres_of=None, clip=True):
    """One self-conditioned step up to the chain's step kernel: (eps_hat, the estimate for the next step, s) with eps_hat =
    to_eps(net(cat([x, est]), t)) (to_eps: the pred_v conversion, in place, or None), s = thres_of(x, t, eps_hat) or None, and the
    estimate restated by x0_estimate on the host from what the device holds."""
    out = net(torch.cat([x, est], dim=1), t)
    eps = out if to_eps is None else to_eps(out, x, t)
    s = None if thres_of is None else thres_of(x, t, eps)
    nxt = x0_estimate(x.cpu(), eps.cpu(), t.cpu(), tables.cpu(), clip=clip, thres=None if s is None else s.cpu())
    return eps, nxt.to(x.device), s
