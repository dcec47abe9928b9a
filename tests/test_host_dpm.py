"""CPU tests of the DPM-Solver++(2M) sampler (EXTENSION, parity unpinned: no reference code): the fp64 restatement in _dpm_ref.py is
pinned against closed forms -- first order is DDIM, second order converges at second order on Gaussian data, whose probability-flow
ODE has an exact solution -- and the host surface rejects bad arguments before any device work."""
import numpy as np
import pytest
import torch

import _dpm_ref as D

T = 1000


def _ac():
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    return torch.from_numpy(make_tables(T)['alphas_cumprod']).double()      # the project's fp32 cosine table, read in fp64


def _x_T():
    return torch.randn(1, 1, 4, 8, 8, generator=torch.Generator().manual_seed(0), dtype=torch.float64)      # 256 elements


def _ddim_closed_form(x, eps, hist, ac, seq, k, order, clip):
    """Song et al. 2020 eq. 12 with eta = 0, as oracle/diffusion_ref.py and ddim_step_kernel spell it."""
    a_t = ac[int(seq[k])]
    a_n = ac[int(seq[k + 1])] if seq[k + 1] >= 0 else torch.ones((), dtype=ac.dtype)
    x0 = (x - (1 - a_t).sqrt() * eps) / a_t.sqrt()
    return a_n.sqrt() * x0 + (1 - a_n).sqrt() * (x - a_t.sqrt() * x0) / (1 - a_t).sqrt(), x0


def test_time_sequence_is_the_projects():
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence
    for S in (1, 10, 20, 1000):
        assert np.array_equal(D.time_sequence(T, S), ddim_time_sequence(T, S))


def test_first_order_is_ddim():
    ac, x_T = _ac(), _x_T()
    for S in (10, 20):
        got = D.gaussian_chain(ac, x_T, S, 1)
        exp = D.gaussian_chain(ac, x_T, S, 1, step=_ddim_closed_form)
        assert (got - exp).abs().max().item() <= 1e-12, S


def test_second_order_converges_on_gaussian_data():
    """sigma^2 = 0.25, no clipping.  Measured with these tables: S = 10 / 20 / 40 first order 0.1464 / 0.0758 / 0.0387, second order
    0.0491 / 0.0030 / 0.0017; the largest extrapolation weight c along the sequences is 0.81."""
    ac, x_T = _ac(), _x_T()
    exact = D.gaussian_exact(x_T, ac[T - 1])
    err = {(o, S): D.rel_err(D.gaussian_chain(ac, x_T, S, o), exact) for o in (1, 2) for S in (10, 20)}
    print('relative L2 error vs the exact ODE solution:', {k: round(v, 4) for k, v in err.items()})
    assert err[2, 20] <= err[1, 20] / 10                # measured ratio 0.040
    assert err[2, 10] / err[2, 20] >= 4                 # measured 16.4; first order gives 1.93
    c_max = max(D.extrapolation_weight(ac, D.time_sequence(T, S), k) for S in (10, 20, 40) for k in range(1, S - 1))
    assert 0.5 <= c_max <= 0.85, c_max


def test_second_order_first_step_and_last_step_are_first_order():
    ac = _ac()
    seq = D.time_sequence(T, 20)
    g = torch.Generator().manual_seed(1)
    x, eps, hist = (torch.randn(2, 1, 2, 4, 4, generator=g, dtype=torch.float64) for _ in range(3))
    for k in (0, 19):
        o1, h1 = D.dpm_step(x, eps, None, ac, seq, k, order=1)
        o2, h2 = D.dpm_step(x, eps, hist, ac, seq, k, order=2)
        assert torch.equal(o1, o2) and torch.equal(h1, h2)
    out, x0 = D.dpm_step(x, eps, hist, ac, seq, 19)
    assert torch.equal(out, x0) and out.abs().max().item() <= 1.0          # the step into the data returns the clipped x0
    assert not torch.equal(D.dpm_step(x, eps, hist, ac, seq, 5, order=2)[0], D.dpm_step(x, eps, hist, ac, seq, 5, order=1)[0])


def test_dpm_arguments_are_rejected_before_any_device_work():
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    gd = GaussianDiffusion(Unet3D(dim=16, rngs=0, channels=1, device='cpu'), image_size=8, num_frames=2, channels=1, timesteps=4)
    video, mask = torch.rand(2, 1, 2, 8, 8), torch.tensor([True, False])
    for kw in (dict(dpm_steps=2, ddim_steps=2), dict(dpm_steps=2, dpm_order=3), dict(dpm_steps=2, dpm_order=0), dict(dpm_steps=0), dict(dpm_steps=5)):
        with pytest.raises(ValueError):
            gd.sample(0, batch_size=2, **kw)
        with pytest.raises(ValueError):
            gd.inpaint(0, video, mask, **kw)
        with pytest.raises(ValueError):
            gd.extend(0, video[:, :, :1], 2, context_frames=1, **kw)
    with pytest.raises(ValueError):
        gd.inpaint(0, video, mask, dpm_steps=2, resample_steps=2)
    with pytest.raises(ValueError):
        gd.extend(0, video[:, :, :1], 2, context_frames=1, dpm_steps=2, resample_steps=2)
    for kw in (dict(steps=0), dict(steps=5), dict(steps=2, order=3)):
        with pytest.raises(ValueError):
            gd.dpm_sample_loop((2, 1, 2, 8, 8), 0, **kw)


def test_sample_cli_dpm_flags():
    import sample
    a = sample.build_parser().parse_args([])
    assert a.dpm_steps is None and a.dpm_order == 2
    a = sample.build_parser().parse_args(['--dpm-steps', '20', '--dpm-order', '1', '--context', 'c.npy'])
    assert (a.dpm_steps, a.dpm_order, a.context, a.ddim_steps) == (20, 1, 'c.npy', None)
    with pytest.raises(SystemExit):
        sample.build_parser().parse_args(['--dpm-steps', '20', '--dpm-order', '3'])
    with pytest.raises(SystemExit):                     # two samplers at once: refused before a model is built
        sample.main(['--random-init', '--dpm-steps', '20', '--ddim-steps', '50', '--config', 'does-not-exist.yaml'])
