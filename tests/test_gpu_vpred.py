"""GPU tests of the v-prediction objective (vdx.h "v-prediction"; GaussianDiffusion(objective='pred_v', min_snr_gamma=...)): the
conversion kernel and the loss pass bit for bit against their fp32 statements in torch and against the fp64 restatement
tests/_vpred_ref.py, every sampling chain captured = replayed = eager = a Python loop over the network, vdx_v_to_eps and the single-step
entries, the launch lists against those of the same network under pred_noise, the bound, the train step and the refusals.
The network is the tiny one of tests/_host_path_cases.py (dim 16, one channel, 4 frames of 8 x 8)."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _host_path_cases as H
import _vlb_ref as VLB
import _vpred_ref as V
from _launch_hook import launches

DEV = 'cuda:0'
F64 = torch.float64
T_TAB = 1000
SEED = H.SEED


def _L():
    from video_diffusion_nnx_amd import _lib as L
    return L


@functools.lru_cache(None)
def _tabs():
    """(sqrt_ac, sqrt_1mac) of the project's T = 1000 schedule on the host (float32) and on the device."""
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables
    t = make_tables(T_TAB)
    sa, s1 = torch.from_numpy(t['sqrt_alphas_cumprod']), torch.from_numpy(t['sqrt_one_minus_alphas_cumprod'])
    return sa, s1, sa.to(DEV), s1.to(DEV)


# the shapes of the kernel tests: (rows, C, fhw).  'odd': per_sample = 65 541 > 4 * 256 * 64 = 65 536, so the grid-stride loop takes
# its second trip; fhw is odd, so quads straddle channels; per_sample % 4 = 1, so the last quad runs the guarded tail.  'vec': one channel,
# float4 loads and stores throughout.  'vecx': three channels with per_sample % 4 = 0, float4 loads of x and scattered stores.
SHAPES = {'odd': (3, 3, 21847), 'vec': (2, 1, 256), 'vecx': (2, 3, 24)}
LEVELS = {'odd': (0, T_TAB - 1, 500), 'vec': (T_TAB - 1, 1), 'vecx': (3, 700)}


@functools.lru_cache(None)
def _case(name):
    """out (channel-last [rows, fhw, C]), x0 in [0, 1], noise, x_t ([rows, C, fhw]) and t of one shape.  Computed once, left unchanged."""
    rows, C, fhw = SHAPES[name]
    g = torch.Generator().manual_seed(31 + len(name))
    return dict(out=torch.randn(rows, fhw, C, generator=g), x0=torch.rand(rows, C, fhw, generator=g), noise=torch.randn(rows, C, fhw, generator=g),
                x=torch.randn(rows, C, fhw, generator=g), t=torch.tensor(LEVELS[name], dtype=torch.int32))


def _col(tab, t):
    return tab[t.long()].reshape(-1, 1, 1)


# ---- 1. vdx_v_to_eps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'x_off_4_bytes'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_v_to_eps_is_the_fp32_expression(name, offset):
    L = _L()
    c = _case(name)
    rows, C, fhw = SHAPES[name]
    sa, s1, sa_d, s1_d = _tabs()
    want = _col(sa, c['t']) * c['out'] + _col(s1, c['t']) * c['x'].permute(0, 2, 1)          # two products and a sum, each rounded to fp32
    buf = torch.full((rows + 1, fhw, C), 7.0, device=DEV)                                    # (one row more: a sentinel behind the rows)
    buf[:rows] = c['out'].to(DEV)
    xbig = torch.empty(rows * C * fhw + 4, device=DEV)
    x = xbig[offset:offset + rows * C * fhw].view(rows, C, fhw)
    x.copy_(c['x'].to(DEV))
    assert x.data_ptr() % 16 == 4 * offset
    keep = x.clone()
    t = c['t'].to(DEV)
    with launches() as rec:
        L.check(L.vdx_v_to_eps(buf.data_ptr(), x.data_ptr(), L.ptr(t), L.ptr(sa_d), L.ptr(s1_d), T_TAB, rows, C, C * fhw, L.stream_ptr()))
        torch.cuda.synchronize()
    assert [k for k, _ in rec] == ['v_to_eps_kernel']
    form = 'scalar' if (offset or (C * fhw) % 4) else 'float4' if C == 1 else 'float4 x'
    assert rec[0][1].endswith(form), rec
    assert torch.equal(buf[:rows].cpu(), want)
    assert (buf[rows] == 7.0).all() and torch.equal(x, keep)


# ---- 2. vdx_v_loss --------------------------------------------------------------------------------------------------------------------------

def _v_loss(c, shape, *, kind, l2, pre, iw, wtab, grad=True):
    L = _L()
    rows, C, fhw = shape
    _, _, sa_d, s1_d = _tabs()
    dev = {k: v.to(DEV) for k, v in c.items()}
    scratch = torch.empty(L.vdx_v_loss_scratch_doubles(rows), dtype=F64, device=DEV)
    result = torch.full((rows + 1,), float('nan'), dtype=F64, device=DEV)
    d_out = torch.full_like(dev['out'], float('nan')) if grad else None
    iw_d, w_d = (None if v is None else v.to(DEV) for v in (iw, wtab))
    with launches() as rec:
        L.check(L.vdx_v_loss(L.ptr(dev['out']), L.ptr(dev['x0']), L.ptr(dev['noise']), L.ptr(dev['t']), L.ptr(sa_d), L.ptr(s1_d), L.ptr(w_d),
                             L.ptr(iw_d), T_TAB, kind, pre[0], pre[1], int(l2), L.ptr(d_out), L.ptr(scratch), L.ptr(result), rows, C, fhw,
                             L.stream_ptr()))
        torch.cuda.synchronize()
    assert [k for k, _ in rec] == ['v_loss_kernel', 'v_loss_final_kernel']
    return result.cpu(), None if d_out is None else d_out.cpu()


def _weights(name):
    """(importance weights [rows], the min-SNR table [T]) of a shape, float64."""
    from video_diffusion_nnx_amd.gaussian_diffusion import min_snr_weights
    rows = SHAPES[name][0]
    return torch.tensor([0.75, 1.0, 2.5][:rows], dtype=F64), torch.from_numpy(min_snr_weights(T_TAB, 'pred_v', 5.0))


@pytest.mark.parametrize('weighted', ['plain', 'iw', 'wtab', 'iw_wtab'])
@pytest.mark.parametrize('pre', [(2.0, -1.0), (1.0, 0.0)], ids=['pre2m1', 'pre10'])
@pytest.mark.parametrize('l2', [False, True], ids=['l1', 'l2'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_v_loss_against_fp32_and_fp64(name, l2, pre, weighted):
    c, shape = _case(name), SHAPES[name]
    rows, C, fhw = shape
    sa, s1, _, _ = _tabs()
    iw_all, w_all = _weights(name)
    iw, wtab = (iw_all if 'iw' in weighted else None), (w_all if 'wtab' in weighted else None)
    result, d_out = _v_loss(c, shape, kind=1, l2=l2, pre=pre, iw=iw, wtab=wtab)
    # the fp32 statement: x0n as q_sample forms it (one fma; with these two pre pairs x0 * scale is exact, so the plain expression is it)
    x0n = c['x0'] * pre[0] + pre[1]
    target = _col(sa, c['t']) * c['noise'] - _col(s1, c['t']) * x0n
    d = c['out'] - target.permute(0, 2, 1)
    w_b = torch.ones(rows, dtype=F64) if wtab is None else wtab[c['t'].long()]
    g_b = (torch.ones(rows, dtype=F64) if iw is None else iw) * w_b
    inv_count = torch.tensor(1.0) / torch.tensor(float(rows * C * fhw))
    f = (g_b.float() * inv_count).reshape(-1, 1, 1)
    want = 2.0 * d * f if l2 else torch.sign(d) * f
    assert not torch.isnan(d_out).any() and torch.equal(d_out, want)
    # the sums in double: the restatement on the same fp32 d; only the order of N = 65 541 double additions differs, N 2^-53 relative
    ref, _ = V.weighted_loss(d.double().numpy(), w_b.numpy(), None if iw is None else iw.numpy(), l2)
    rel = np.abs(result.numpy() - ref) / np.abs(ref)
    print(f'[{name} l2 {l2} pre {pre} {weighted}] result {result.tolist()}  relative error {rel.tolist()}')
    assert (rel <= 1e-10).all()
    again, d_again = _v_loss(c, shape, kind=1, l2=l2, pre=pre, iw=iw, wtab=wtab)
    assert torch.equal(result.view(torch.int64), again.view(torch.int64)) and torch.equal(d_out.view(torch.int32), d_again.view(torch.int32))
    if weighted == 'plain':
        none, no_grad = _v_loss(c, shape, kind=1, l2=l2, pre=pre, iw=iw, wtab=wtab, grad=False)
        assert no_grad is None and torch.equal(none, result)


@pytest.mark.parametrize('with_iw', [False, True], ids=['plain', 'iw'])
@pytest.mark.parametrize('l2', [False, True], ids=['l1', 'l2'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_v_loss_kind0_is_loss_weighted(name, l2, with_iw):
    """Target noise, no level weights: vdx_loss_weighted's result and gradient bit for bit; with level weights, the restatement."""
    from video_diffusion_nnx_amd import timestep_sampler as TS
    c, shape = _case(name), SHAPES[name]
    rows, C, fhw = shape
    iw_all, w_all = _weights(name)
    iw = iw_all if with_iw else None
    result, d_out = _v_loss(c, shape, kind=0, l2=l2, pre=(2.0, -1.0), iw=iw, wtab=None)
    noise5 = c['noise'].reshape(rows, C, 1, 1, fhw).to(DEV)
    ref, d_ref = TS.loss_weighted(c['out'].to(DEV), noise5, None if iw is None else iw.to(DEV), l2=l2, want_grad=True)
    assert torch.equal(result.view(torch.int64), ref.cpu().view(torch.int64))
    assert torch.equal(d_out.view(torch.int32), d_ref.cpu().view(torch.int32))
    # min-SNR weighting of the eps objective
    got, g_out = _v_loss(c, shape, kind=0, l2=l2, pre=(2.0, -1.0), iw=iw, wtab=w_all)
    d = c['out'] - c['noise'].permute(0, 2, 1)
    w_b = w_all[c['t'].long()]
    want, _ = V.weighted_loss(d.double().numpy(), w_b.numpy(), None if iw is None else iw.numpy(), l2)
    assert (np.abs(got.numpy() - want) <= 1e-10 * np.abs(want)).all()
    f = ((w_b if iw is None else iw * w_b).float() * (torch.tensor(1.0) / torch.tensor(float(rows * C * fhw)))).reshape(-1, 1, 1)
    assert torch.equal(g_out, 2.0 * d * f if l2 else torch.sign(d) * f)


# ---- 3. the chains --------------------------------------------------------------------------------------------------------------------------

S = H.S
B = H.B


def _pair(kind, **gkw):
    """(pred_noise diffusion, pred_v diffusion) over ONE network of the rig."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    e = H._gd(kind, **gkw)
    kw = dict(gkw)
    if kind in ('mixed', 'mixed_cond'):
        kw['frame_noise_alpha'] = 1.0
    if kind == 'sr':
        kw.setdefault('lowres_cond', (2, 2))
    v = GaussianDiffusion(e.denoise_fn, image_size=8, num_frames=4, channels=1, timesteps=H.T, objective='pred_v', **kw)
    return e, v


def _loop(gd, chain, **kw):
    if chain == 'ddpm':
        return gd.p_sample_loop(H.SHAPE, SEED, **kw)
    if chain == 'ddim':
        return gd.ddim_sample_loop(H.SHAPE, SEED, steps=S, **kw)
    return gd.dpm_sample_loop(H.SHAPE, SEED, steps=S, order=2, **kw)


def _call(gd, chain, variant, use_graph):
    if variant == 'guided':
        return _loop(gd, chain, cond=H._cond(), cond_scale=2.0, guidance_rescale=0.5, use_graph=use_graph)
    if variant == 'masked':
        steps = {'ddpm': {}, 'ddim': dict(ddim_steps=S), 'dpm': dict(dpm_steps=S)}[chain]
        return gd.inpaint(SEED, H._video(), H.HALF, use_graph=use_graph, **steps)
    if variant == 'sr':
        return gd.upsample(SEED, H._lowres(), use_graph=use_graph)
    return _loop(gd, chain, use_graph=use_graph)


def _python_chain(gd, chain, variant):
    """The chain as a Python loop: the network, vdx_v_to_eps (through _eps_from_out, or over the 2B rows of a guided batch before
    vdx_cfg_combine) and the single-step entries, with the draws of the captured loops."""
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    L = _L()
    unet, T, C = gd.denoise_fn, gd.num_timesteps, gd.channels
    st = L.stream_ptr
    img = gd.noise(H.SHAPE, SEED, 0)
    per = img[0].numel()
    seq_host = None if chain == 'ddpm' else G.ddim_time_sequence(T, S)
    seq = None if seq_host is None else torch.from_numpy(seq_host).to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist = torch.empty_like(img) if chain == 'dpm' else None
    unnorm = lambda x: x * 0.5 + 0.5
    if variant == 'masked':
        known, mk = torch.empty_like(img), G.frame_mask(H.HALF, H.SHAPE).to(DEV)
        t0 = T - 1 if seq_host is None else int(seq_host[0])
        L.check(G.vdx_affine(L.ptr(H._video().to(DEV)), L.ptr(known), img.numel(), 2.0, -1.0, st()))
        L.check(G.vdx_inpaint_init(L.ptr(img), L.ptr(known), L.ptr(mk), L.ptr(gd._mtab), T, t0, img.numel(), st()))
        gd._masked_guided_steps(chain, dict(img=img, known=known, mask=mk, hist=hist, seq=seq, step=step), seq_host, None, 1.0, 2, 1, gd._mtab, SEED)
        return unnorm(img)
    xin = None
    if variant == 'sr':
        xin = torch.zeros(B, 2 * C, *H.SHAPE[2:], device=DEV)
        gd.lowres_condition(H._lowres(), SEED, None, draw=L.DRAW_LOWRES, out=xin)
    cond = H._cond().to(DEV) if variant == 'guided' else None
    scratch = torch.empty(L.vdx_cfg_scratch_doubles(B), dtype=F64, device=DEV) if variant == 'guided' else None
    null = torch.zeros(2 * B, dtype=torch.bool, device=DEV)
    null[B:] = True
    levels = list(range(T - 1, -1, -1)) if chain == 'ddpm' else [int(t) for t in seq_host[:-1]]
    for k, lv in enumerate(levels):
        t = torch.full((B,), lv, dtype=torch.int32, device=DEV)
        if variant == 'guided':
            x2, t2 = torch.cat((img, img)), torch.cat((t, t))
            out = unet(x2, t2, torch.cat((cond, cond)), cond_mask=null)
            L.check(L.vdx_v_to_eps(L.ptr(out), L.ptr(x2), L.ptr(t2), L.ptr(gd.sqrt_alphas_cumprod), L.ptr(gd.sqrt_one_minus_alphas_cumprod), T,
                                   2 * B, C, per, st()))
            L.check(L.vdx_cfg_combine(L.ptr(out), L.ptr(out), 2.0, 0.5, L.ptr(scratch), B, per, st()))
            eps = out[:B]
        elif variant == 'sr':
            xin[:, :C] = img
            eps = gd._eps_from_out(unet(xin, t), img, t)
        else:
            eps = gd._eps_from_out(unet(img, t), img, t)
        th = gd._dynamic_threshold(img, t, eps) if gd.use_dynamic_thres else None
        new = torch.empty_like(img)
        tail = (B, C, per, st())
        if chain == 'ddpm' and gd.frame_noise_alpha:
            L.check(L.vdx_p_sample_step_mixed(L.ptr(img), L.ptr(eps), L.ptr(new), L.ptr(t), L.ptr(gd._ptab), T, img.shape[2], gd._mix[0], gd._mix[1],
                                              SEED, 1 + k, 0, L.ptr(th), 1, *tail))
        elif chain == 'ddpm':
            L.check(G.vdx_p_sample_step(L.ptr(img), L.ptr(eps), L.ptr(new), L.ptr(t), L.ptr(gd._ptab), T, None, SEED, 1 + k, 0, L.ptr(th), 1, *tail))
        elif chain == 'ddim':
            step.fill_(k)
            L.check(G.vdx_ddim_step(L.ptr(img), L.ptr(eps), L.ptr(new), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step), L.ptr(th), 1, *tail))
        else:
            step.fill_(k)
            L.check(G.vdx_dpm_step(L.ptr(img), L.ptr(eps), L.ptr(new), L.ptr(hist), L.ptr(gd.alphas_cumprod), L.ptr(seq), L.ptr(step), L.ptr(th),
                                   1, 2, *tail))
        img = new
    out = torch.empty_like(img)
    L.check(G.vdx_affine(L.ptr(img), L.ptr(out), img.numel(), 0.5, 0.5, st()))
    return out


def _with_conversion(rec):
    """A pred_noise launch list with v_to_eps_kernel directly behind every forward's last launch."""
    out = []
    for k in (k for k, _ in rec):
        out.append(k)
        if k.startswith('final_conv'):
            out.append('v_to_eps_kernel')
    return out


def _run(gd, chain, variant, use_graph):
    torch.cuda.synchronize()
    with launches() as rec:
        out = _call(gd, chain, variant, use_graph)
        torch.cuda.synchronize()
    return list(rec), out.cpu().clone()


CHAINS = [(c, v, k, {}) for c in ('ddpm', 'ddim', 'dpm') for v, k in (('plain', 'plain'), ('guided', 'cond'), ('masked', 'plain'))]
CHAINS += [('ddpm', 'plain', 'mixed', {}), ('ddpm', 'sr', 'sr', {}), ('ddim', 'plain', 'plain', dict(use_dynamic_thres=True))]


@pytest.mark.parametrize('chain,variant,kind,gkw', CHAINS, ids=[f'{c}-{v}-{k}{"-dyn" if g else ""}' for c, v, k, g in CHAINS])
def test_chain_captured_replayed_eager_and_launch_lists(chain, variant, kind, gkw):
    gd_e, gd_v = _pair(kind, **gkw)
    unet = gd_e.denoise_fn
    # pred_noise first: the bits and the lists the switch has to give back
    e_eager, e_out0 = _run(gd_e, chain, variant, False)
    e_graph, e_out = _run(gd_e, chain, variant, True)
    assert torch.equal(e_out0, e_out) and 'v_to_eps_kernel' not in [k for k, _ in e_eager + e_graph]
    # pred_v on the same network: eager, captured, replayed
    v_eager, out_eager = _run(gd_v, chain, variant, False)
    v_graph, out_graph = _run(gd_v, chain, variant, True)
    v_replay, out_replay = _run(gd_v, chain, variant, True)
    assert torch.isfinite(out_graph).all() and not torch.equal(out_graph, e_out)
    assert torch.equal(out_eager, out_graph) and torch.equal(out_graph, out_replay)
    assert [k for k, _ in v_eager] == _with_conversion(e_eager)
    assert [k for k, _ in v_graph] == _with_conversion(e_graph)
    assert H.forwards(v_graph) > 0 and H.forwards(v_replay) == 0 and 'v_to_eps_kernel' not in [k for k, _ in v_replay]
    # the Python loop over the network, vdx_v_to_eps and the single-step entries
    with gd_v._sampling(None, B):
        py = _python_chain(gd_v, chain, variant)
        torch.cuda.synchronize()
    assert torch.equal(py.cpu(), out_graph)
    h = unet.handle(4, 8)
    assert _L().vdx_get_prediction(h.ptr) == 0                                 # (put back on the way out of every loop)
    # back to pred_noise on the same network: a new capture, the bits and the list from before the switch
    e_again, e_out2 = _run(gd_e, chain, variant, True)
    assert torch.equal(e_out2, e_out)
    assert [k for k, _ in e_again] == [k for k, _ in e_graph] and H.forwards(e_again) > 0


# ---- 4. the bound ---------------------------------------------------------------------------------------------------------------------------

def test_calc_bpd_loop_on_a_v_predicting_diffusion():
    from video_diffusion_nnx_amd import ops
    from video_diffusion_nnx_amd.gaussian_diffusion import make_vlb_tables, vdx_randn
    L = _L()
    gd_e, gd = _pair('plain')
    unet, T = gd.denoise_fn, gd.num_timesteps
    x = H._video()
    with launches() as rec:
        cap = gd.calc_bpd_loop(x, SEED)
    eager = gd.calc_bpd_loop(x, SEED, use_graph=False)
    keys = ('vb', 'mse', 'xstart_mse', 'prior_bpd', 'total_bpd', 't')
    assert all(torch.equal(cap[k], eager[k]) for k in keys) and all(torch.isfinite(cap[k]).all() for k in keys)
    names = [k for k, _ in rec]
    assert names.count('v_to_eps_kernel') == 2 and all(names[i + 1] == 'v_to_eps_kernel' for i, k in enumerate(names) if k.startswith('final_conv'))
    plain = gd_e.calc_bpd_loop(x, SEED)
    assert torch.equal(plain['prior_bpd'], cap['prior_bpd']) and not torch.equal(plain['vb'], cap['vb'])
    # the pred_noise restatement fed the converted eps_hat, level by level, at the bound of tests/test_gpu_vlb.py: 8 x the error of the
    # same restatement evaluated in fp32
    tab_host = make_vlb_tables(T)
    tab, xd = torch.from_numpy(tab_host).to(DEV), x.to(DEV)
    for k, lv in enumerate(range(T - 1, -1, -1)):
        t = torch.full((B,), lv, dtype=torch.int32, device=DEV)
        z = torch.empty(H.SHAPE, device=DEV)
        L.check(vdx_randn(L.ptr(z), z.numel(), SEED, 1 + k, 0, L.stream_ptr()))
        xt = ops.vlb_noise(xd, t, tab, seed=SEED, draw=1 + k)
        eps_hat = gd._eps_from_out(unet(xt, t), xt, t)
        step = ops.vlb_terms(xd, eps_hat, t, tab, seed=SEED, draw=1 + k).cpu()
        for j, key in enumerate(('vb', 'mse', 'xstart_mse')):
            assert torch.equal(step[:, j], cap[key][:, k]), (key, k)                       # the loop is the single-step entries
        args = (x, VLB.cf(eps_hat.cpu()), z.cpu(), t.cpu(), tab_host)
        ref, ref32 = VLB.terms(*args), VLB.terms(*args, dt=VLB.F32)
        bound = VLB.term_bounds(ref32, ref, t.cpu())
        for j, key in enumerate(('vb', 'mse', 'xstart_mse')):
            err = (cap[key][:, k] - ref[j]).abs()
            print(f'[bpd pred_v t = {lv}] {key}: value {ref[j].tolist()}  error {err.tolist()}  bound {bound[j].tolist()}')
            assert (err <= bound[j]).all(), (key, lv)


# ---- 5. the train step ----------------------------------------------------------------------------------------------------------------------

LOSS_LAUNCHES = ('loss_grad_kernel', 'loss_weighted_kernel', 'loss_weighted_final_kernel')


def _train_two_steps(sampler, **gkw):
    """Two optimizer steps -> (launches of step 0, [loss0, grads0, loss1, grads1] on the host, the device pieces of step 0's objective)."""
    from video_diffusion_nnx_amd.train_step import run_train_step
    gd = H._gd('plain', **gkw)
    unet = gd.denoise_fn
    batch = H._video()
    with tempfile.TemporaryDirectory() as tmp:
        tr = H._trainer(gd, dict(timestep_sampler='loss-second-moment') if sampler else {}, tmp)
        p0 = unet.flat_params.clone()
        torch.cuda.synchronize()
        with launches() as rec:
            loss0 = run_train_step(tr, batch, 0)
            torch.cuda.synchronize()
        outs = [loss0.cpu().clone(), tr.grads.cpu().clone()]
        t, noise = tr.last_t.clone(), gd.noise(H.SHAPE, tr.last_noise_key, 0)
        iw = None if tr.last_iw is None else tr.last_iw.clone()
        per_sample = gd.last_loss_per_sample.cpu().clone() if hasattr(gd, 'last_loss_per_sample') else None
        loss1 = run_train_step(tr, batch.flip(0), 1)
        torch.cuda.synchronize()
        outs += [loss1.cpu().clone(), tr.grads.cpu().clone()]
        # the objective of step 0 again, on the parameters the step started from
        p1 = unet.flat_params.clone()
        unet.flat_params.copy_(p0)
        unet.mark_params_updated()
        xd = batch.to(DEV)
        out = unet(gd.q_sample(xd, t, noise=noise, _pre=(2.0, -1.0)), t)
        loss, d_out = gd.loss_and_grad(out, xd, noise, t, iw=iw, want_grad=True, _pre=(2.0, -1.0))
        torch.cuda.synchronize()
        unet.flat_params.copy_(p1)
        unet.mark_params_updated()
        pieces = dict(out=out.cpu(), x=batch, noise=noise.cpu(), t=t.cpu(), iw=None if iw is None else iw.cpu(), loss=loss.cpu(), d_out=d_out.cpu(),
                      per_sample=per_sample, result=gd.last_loss_per_sample.cpu() if hasattr(gd, 'last_loss_per_sample') else None)
    return list(rec), outs, pieces


@pytest.mark.parametrize('sampler', [False, True], ids=['uniform', 'loss_second_moment'])
def test_train_step_pred_v_min_snr(sampler):
    from video_diffusion_nnx_amd.gaussian_diffusion import make_tables, min_snr_weights
    rec, outs, p = _train_two_steps(sampler, objective='pred_v', min_snr_gamma=5.0)
    assert all(torch.isfinite(o).all() for o in outs) and outs[1].abs().max() > 0
    # the loss and its gradient on the network's own output: the fp32 statement bit for bit, the sums against the restatement
    tabs = make_tables(H.T)
    sa, s1 = torch.from_numpy(tabs['sqrt_alphas_cumprod']), torch.from_numpy(tabs['sqrt_one_minus_alphas_cumprod'])
    col = lambda tab: tab[p['t'].long()].reshape(-1, 1, 1, 1, 1)
    target = col(sa) * p['noise'] - col(s1) * (p['x'] * 2.0 - 1.0)
    d = p['out'] - target.permute(0, 2, 3, 4, 1)
    w_b = torch.from_numpy(min_snr_weights(H.T, 'pred_v', 5.0))[p['t'].long()]
    iw = torch.ones(B, dtype=F64) if p['iw'] is None else p['iw']
    f = ((iw * w_b).float() * (torch.tensor(1.0) / torch.tensor(float(d.numel())))).reshape(-1, 1, 1, 1, 1)
    assert torch.equal(p['d_out'], torch.sign(d) * f)
    ref, _ = V.weighted_loss(d.double().numpy(), w_b.numpy(), iw.numpy(), False)
    assert (np.abs(p['result'].numpy() - ref[:B]) <= 1e-10 * np.abs(ref[:B])).all()
    assert abs(float(p['loss']) - ref[B]) <= 2.0 ** -23 * abs(ref[B])                      # (the double total, rounded to fp32 once)
    assert torch.equal(p['loss'], outs[0]) and torch.equal(p['result'], p['per_sample'])  # what the step returned and kept
    # bit-reproducible run to run
    rec2, outs2, _ = _train_two_steps(sampler, objective='pred_v', min_snr_gamma=5.0)
    assert [k for k, _ in rec2] == [k for k, _ in rec] and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, outs2))
    # the launch list: v_loss_kernel and its final in place of the loss launches of the same trainer under pred_noise
    rec_e, outs_e, _ = _train_two_steps(sampler)
    names, names_e = [k for k, _ in rec], [k for k, _ in rec_e]
    assert not any(k.startswith('v_') for k in names_e)
    want, i = [], 0
    while i < len(names_e):
        if names_e[i] in LOSS_LAUNCHES:
            want += ['v_loss_kernel', 'v_loss_final_kernel']
            while i < len(names_e) and names_e[i] in LOSS_LAUNCHES:
                i += 1
        else:
            want.append(names_e[i])
            i += 1
    assert names == want and names.count('v_loss_kernel') == 1
    assert not torch.equal(outs_e[1], outs[1])
    if not sampler:
        # ... and that pred_noise list is the one the tree has always recorded for this trainer
        doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_path_launches.json')))
        assert rec_e == H.decode(doc, 'train/l1')


def test_min_snr_on_the_eps_objective():
    """pred_noise with gamma: the same pass with target noise; without gamma nothing of it runs (above)."""
    from video_diffusion_nnx_amd.gaussian_diffusion import min_snr_weights
    rec, outs, p = _train_two_steps(False, min_snr_gamma=5.0)
    assert [k for k, _ in rec].count('v_loss_kernel') == 1 and 'loss_grad_kernel' not in [k for k, _ in rec]
    d = p['out'] - p['noise'].permute(0, 2, 3, 4, 1)
    w_b = torch.from_numpy(min_snr_weights(H.T, 'pred_noise', 5.0))[p['t'].long()]
    f = (w_b.float() * (torch.tensor(1.0) / torch.tensor(float(d.numel())))).reshape(-1, 1, 1, 1, 1)
    assert torch.equal(p['d_out'], torch.sign(d) * f)
    ref, _ = V.weighted_loss(d.double().numpy(), w_b.numpy(), None, False)
    assert (np.abs(p['result'].numpy() - ref[:B]) <= 1e-10 * np.abs(ref[:B])).all() and torch.equal(p['loss'], outs[0])


# ---- 6. refusals on the device --------------------------------------------------------------------------------------------------------------

def test_lv_loops_refuse_a_v_predicting_handle_on_the_device():
    L = _L()
    gd = H._gd('lv')
    unet = gd.denoise_fn
    h = unet.handle(4, 8)
    L.check(L.vdx_set_prediction(h.ptr, 1, L.ptr(gd.sqrt_alphas_cumprod), L.ptr(gd.sqrt_one_minus_alphas_cumprod), gd.num_timesteps))
    try:
        with launches() as rec:
            with pytest.raises(L.VdxError, match='status -4: p_sample_loop_lv: v-prediction'):
                gd.p_sample_loop(H.SHAPE, SEED)
            with pytest.raises(L.VdxError, match='status -4: vlb_loop_lv: v-prediction'):
                gd.calc_bpd_loop(H._video(), SEED)
            torch.cuda.synchronize()
        names = [k for k, _ in rec]
        assert H.forwards(rec) == 0 and 'p_sample_lv_kernel' not in names and 'vlb_term_lv_kernel' not in names      # no step was launched
    finally:
        L.check(L.vdx_set_prediction(h.ptr, 0, None, None, 0))
    assert torch.isfinite(gd.p_sample_loop(H.SHAPE, SEED)).all()
