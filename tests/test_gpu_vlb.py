"""GPU tests of the held-out evaluation (vdx.h "Held-out evaluation"; GaussianDiffusion.calc_bpd_loop; evaluate.py): the two fused
kernels against the fp64 restatement tests/_vlb_ref.py at the shapes where they can go wrong, the captured loop against the eager one,
against a Python loop over the single-step entries and against the restatement fed with the fp64 oracle network, its graph slot beside
the sampling loops', and the command-line tool.  Every bound is 8 x the error of the same restatement evaluated in fp32 on the CPU (or,
for the loop, fed with the fp32 oracle network), computed here and printed beside the measured figure; tests/test_host_vlb.py proves
that each of them can tell a wrong kernel."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _vlb_ref as V
from _launch_hook import assert_launches, launches, nan_outputs
from oracle import philox_ref, unet3d_ref as R

DEV = 'cuda:0'
F64 = torch.float64
U24 = 2.0 ** -24
RANDN_ATOL, RANDN_RTOL = 3e-6, 1e-5          # the device's Philox normals against oracle/philox_ref (tests/_step_cases.py)
SEED = 7


def _ops():
    from video_diffusion_nnx_amd import ops
    return ops


@functools.lru_cache(None)
def _tab(T=V.T_CASE):
    return torch.from_numpy(V.tables(T)).to(DEV)


@functools.lru_cache(None)
def _dev_case(name):
    c = V.case(name)
    return {k: c[k].to(DEV) for k in ('x', 'eps', 'eps_hat', 't')}


def _device_randn(shape, seed, draw):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_randn
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    L.check(vdx_randn(L.ptr(out), out.numel(), seed, draw, 0, L.stream_ptr()))
    return out


def _xt_bound(ref64, extra=0.0):
    """The one-fma bound of tests/test_gpu_step_kernels.py: one correctly rounded result, 2^-24 |ref| (1 + 1e-9).  vlb_noise_kernel forms
    x_t in double (exact products, one double rounding) and rounds it to fp32 once."""
    return U24 * ref64.abs() * (1 + 1e-9) + extra


def _check_terms(got, name, clip, what, ref=None, ref32=None):
    c = V.case(name)
    ref = V.case_ref(name, clip) if ref is None else ref
    ref32 = V.case_ref(name, clip, V.F32) if ref32 is None else ref32
    bound = V.term_bounds(ref32, ref, c['t'])
    got = got.cpu()
    assert not torch.isnan(got).any(), f'{what}: NaN sentinel left'
    err = torch.stack([(got[:, k] - ref[k]).abs() for k in range(3)])
    for k, q in enumerate(('vb', 'mse', 'xstart_mse')):
        print(f'[{what}] {q}: value {[f"{v:.6e}" for v in ref[k].tolist()]}  error {[f"{v:.2e}" for v in err[k].tolist()]}  '
              f'bound {[f"{v:.2e}" for v in bound[k].tolist()]}  error / bound {(err[k] / bound[k]).max().item():.3f}')
    assert (err <= bound).all(), (what, err.tolist(), bound.tolist())


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(V.CASES))
def test_noise_and_terms_with_explicit_noise(name):
    """x_t against the one-fma bound 2^-24 |ref|; the three terms against 8 x the fp32 floor.  Measured on an MI355X: DESIGN.md (section 8)."""
    ops, c, d = _ops(), V.case(name), _dev_case(name)
    B, per = c['shape'][0], c['x'].numel() // c['shape'][0]
    with launches() as rec, nan_outputs():
        xt = ops.vlb_noise(d['x'], d['t'], _tab(), noise=d['eps'])
    assert_launches(rec, [('vlb_noise_kernel', [f'B{B} px{per}', 'noise'])], name)
    ref = V.x_t(c['x'], c['eps'], c['t'], V.tables())
    err = (xt.cpu().double() - ref).abs()
    assert not torch.isnan(xt).any()
    print(f'[x_t {name}] worst error / bound {(err / _xt_bound(ref)).max().item():.3f}  max error {err.max().item():.3e}')
    assert (err <= _xt_bound(ref)).all()
    for clip in (True, False):
        with launches() as rec, nan_outputs():
            got = ops.vlb_terms(d['x'], d['eps_hat'], d['t'], _tab(), noise=d['eps'], clip=clip)
        assert_launches(rec, [('vlb_term_kernel', [f'B{B} px{per} C{c["shape"][1]}', 'noise', f'clip{int(clip)}']), ('vlb_advance_kernel', [f'B{B} n3'])], name)
        _check_terms(got, name, clip, f'terms {name} clip={clip}')
    col = lambda row: torch.from_numpy(V.tables()[row])[c['t'].long()].reshape(-1, 1, 1, 1, 1)
    xh = col(2) * ref - col(3) * V.cf(c['eps_hat']).double()              # with the clip on some |x0_hat| > 1 were cut, some were not
    assert (xh.abs() > 1).any() and (xh.abs() < 1).any()
    assert torch.equal(d['x'].cpu(), c['x']) and torch.equal(d['eps_hat'].cpu(), c['eps_hat'])


@pytest.mark.parametrize('name', list(V.CASES))
def test_philox_form(name):
    """The in-kernel draw: the bits of vdx_randn's stream (so the explicit-noise form on that tensor gives the same bits), the values of
    oracle/philox_ref, and draw + *step_dev."""
    ops, c, d = _ops(), V.case(name), _dev_case(name)
    shape, n = c['shape'], c['x'].numel()
    z_dev = _device_randn(shape, SEED, 3)
    z_ref = torch.from_numpy(philox_ref.randn(n, SEED, 3)).reshape(shape)
    with launches() as rec, nan_outputs():
        xt = ops.vlb_noise(d['x'], d['t'], _tab(), seed=SEED, draw=3)
    assert_launches(rec, [('vlb_noise_kernel', ['philox'])], name)
    assert torch.equal(xt, ops.vlb_noise(d['x'], d['t'], _tab(), noise=z_dev))
    ref = V.x_t(c['x'], z_ref, c['t'], V.tables())
    s = torch.from_numpy(V.tables()[1])[c['t'].long()].reshape(-1, 1, 1, 1, 1)
    bound = _xt_bound(ref, extra=s * (RANDN_ATOL + RANDN_RTOL * z_ref.double().abs()))      # (the device's normals against the CPU's)
    err = (xt.cpu().double() - ref).abs()
    print(f'[x_t philox {name}] worst error / bound {(err / bound).max().item():.3f}')
    assert (err <= bound).all()
    step = torch.tensor([2], dtype=torch.int64, device=DEV)
    assert torch.equal(xt, ops.vlb_noise(d['x'], d['t'], _tab(), seed=SEED, draw=1, step_dev=step))
    for clip in (True, False):
        with launches() as rec, nan_outputs():
            got = ops.vlb_terms(d['x'], d['eps_hat'], d['t'], _tab(), seed=SEED, draw=3, clip=clip)
        assert_launches(rec, [('vlb_term_kernel', ['philox']), ('vlb_advance_kernel', [])], name)
        assert torch.equal(got, ops.vlb_terms(d['x'], d['eps_hat'], d['t'], _tab(), noise=z_dev, clip=clip))
        assert torch.equal(got, ops.vlb_terms(d['x'], d['eps_hat'], d['t'], _tab(), seed=SEED, draw=1, step_dev=step, clip=clip))
        # the values: the restatement on the device's own draw (its bits were held to philox_ref's values above)
        zc = z_dev.cpu()
        _check_terms(got, name, clip, f'terms philox {name} clip={clip}', ref=V.terms(c['x'], V.cf(c['eps_hat']), zc, c['t'], V.tables(), clip),
                     ref32=V.terms(c['x'], V.cf(c['eps_hat']), zc, c['t'], V.tables(), clip, V.F32))


@pytest.mark.parametrize('name', list(V.CASES))
@pytest.mark.parametrize('T', [V.T_CASE, 50])
def test_prior(name, T):
    ops, c, d = _ops(), V.case(name), _dev_case(name)
    with launches() as rec, nan_outputs():
        got = ops.vlb_prior(d['x'], _tab(T))
    assert_launches(rec, [('vlb_prior_kernel', [f'B{c["shape"][0]}']), ('vlb_advance_kernel', ['n1'])], name)
    ref, ref32 = V.prior(c['x'], V.tables(T)), V.prior(c['x'], V.tables(T), V.F32)
    bound = 8.0 * V.rel(ref32, ref).max() * ref.abs()
    err = (got.cpu() - ref).abs()
    print(f'[prior {name} T={T}] value {ref.tolist()}  error {err.tolist()}  bound {bound.tolist()}')
    assert not torch.isnan(got).any() and (err <= bound).all()


def test_terms_are_bit_reproducible():
    ops, d = _ops(), _dev_case('WRAP')
    runs = [ops.vlb_terms(d['x'], d['eps_hat'], d['t'], _tab(), seed=SEED, draw=1).cpu() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert torch.equal(runs[0].view(torch.int64), runs[2].view(torch.int64))


# ---- 2. the loop ----------------------------------------------------------------------------------------------------------------------

T_LOOP = 50
NETS = {'c1': (dict(dim=16, channels=1, dim_mults=(1, 2)), (2, 1, 2, 32, 32)),      # the network of tests/test_gpu_long_attention_backward.py
        'c3': (dict(dim=16, channels=3, dim_mults=(1, 2)), (2, 3, 2, 16, 16))}


class Rig:
    def __init__(self, net, mode='f32'):
        from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
        from video_diffusion_nnx_amd.unet3d import Unet3D
        kw, self.shape = NETS[net]
        self.cfg = R.UnetConfig(**kw)
        self.params = R.random_params(self.cfg, seed=1, dtype=F64)
        self.unet = Unet3D(rngs=0, mode=mode, **kw)
        self.unet.load_state_dict({k: v.float() for k, v in self.params.items()})
        self.gd = GaussianDiffusion(self.unet, image_size=self.shape[3], num_frames=self.shape[2], channels=self.shape[1], timesteps=T_LOOP)
        g = torch.Generator().manual_seed(21)
        self.x = torch.rand(self.shape, generator=g)
        self.tab = V.tables(T_LOOP)

    def run(self, **kw):
        pieces = kw.pop('pieces', None)
        args = dict(cond=None, clip_denoised=True, timesteps=None, use_graph=True, focus_present=None)
        args.update(kw)
        return self.gd._bpd_chain(self.x, SEED, args['cond'], args['clip_denoised'], args['timesteps'], args['use_graph'], args['focus_present'], pieces)


@functools.lru_cache(None)
def rig(net, mode='f32'):
    return Rig(net, mode)


@functools.lru_cache(None)
def captured(net):
    return rig(net).run()


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('vb', 'mse', 'xstart_mse', 'prior_bpd', 'total_bpd', 't'))


@pytest.mark.parametrize('net', list(NETS))
def test_captured_loop_equals_eager_and_pieces(net):
    r, cap = rig(net), captured(net)
    assert all(torch.isfinite(cap[k]).all() for k in ('vb', 'mse', 'xstart_mse', 'prior_bpd', 'total_bpd'))
    assert _same(cap, r.run(use_graph=False))
    assert _same(cap, r.run(pieces=(20, 30)))
    assert _same(cap, r.run(pieces=(1, 0, 48, 1)))


@pytest.mark.parametrize('net', list(NETS))
def test_loop_equals_python_loop_over_single_steps(net):
    ops, r, cap = _ops(), rig(net), captured(net)
    B = r.shape[0]
    x, tab = r.x.to(DEV), torch.from_numpy(r.tab).to(DEV)
    rows = []
    for k, t in enumerate(range(T_LOOP - 1, -1, -1)):
        tt = torch.full((B,), t, dtype=torch.int32, device=DEV)
        xt = ops.vlb_noise(x, tt, tab, seed=SEED, draw=1 + k)
        rows.append(ops.vlb_terms(x, r.unet(xt, tt), tt, tab, seed=SEED, draw=1 + k).cpu())
    out = torch.stack(rows, 1)                                            # [B,S,3]
    for j, key in enumerate(('vb', 'mse', 'xstart_mse')):
        assert torch.equal(out[:, :, j], cap[key]), key
    assert torch.equal(ops.vlb_prior(x, tab).cpu(), cap['prior_bpd'])


# the steps held against the oracle network: every one at 16 x 16; at 32 x 32, where the batched fp64 forward on the CPU is the whole cost
# of the test (0.2 s per step), both ends, the decoder and every third step between
ORACLE_STEPS = {'c1': tuple(sorted(set(range(0, T_LOOP, 3)) | {1, T_LOOP - 3, T_LOOP - 2, T_LOOP - 1})), 'c3': tuple(range(T_LOOP))}


@functools.lru_cache(None)
def oracle_terms(net):
    """The restatement at the steps ORACLE_STEPS[net], fed with the oracle network in fp64 and in fp32: the forwards as one batch (x_t of
    a level does not depend on the level before).  ([3][B,K] fp64-fed, [3][B,K] fp32-fed, t [K], steps [K])."""
    r = rig(net)
    B, n = r.shape[0], int(np.prod(r.shape))
    ks = torch.tensor(ORACLE_STEPS[net])
    K = len(ks)
    ts = T_LOOP - 1 - ks
    eps = torch.stack([torch.from_numpy(philox_ref.randn(n, SEED, 1 + int(k))).reshape(r.shape) for k in ks])      # [K,B,...]
    x_all = r.x.unsqueeze(0).expand(K, *r.shape).reshape(-1, *r.shape[1:])
    t_all = ts.repeat_interleave(B)
    e_all = eps.reshape(-1, *r.shape[1:])
    xt = V.x_t(x_all, e_all, t_all, r.tab)
    with torch.no_grad():
        eh64 = V.cf(R.unet_forward(r.params, r.cfg, xt, t_all))
        p32 = {k: v.float() for k, v in r.params.items()}
        eh32 = V.cf(R.unet_forward(p32, r.cfg, xt.float(), t_all))
    fold = lambda v: v.reshape(K, B).t().contiguous()
    return ([fold(v) for v in V.terms(x_all, eh64, e_all, t_all, r.tab)], [fold(v) for v in V.terms(x_all, eh32, e_all, t_all, r.tab)], ts, ks)


@pytest.mark.parametrize('net', list(NETS))
def test_loop_against_the_oracle_network(net):
    """The loop's out against the restatement fed with the fp64 oracle network.  channels = 3 at 16 x 16: all 50 steps.  channels = 1 at
    32 x 32: the 20 steps of ORACLE_STEPS (both ends, the decoder, every third step) -- the batched fp64 forward on the CPU costs 0.2 s
    per step, 10 s for all 50; the 30 other steps have no independent reference at this shape, only the bit-equality with the Python loop
    over the single-step entries.  Figures measured on the MI355X are in DESIGN.md (section 8)."""
    r, cap = rig(net), captured(net)
    ref, ref32, ts, ks = oracle_terms(net)
    B = r.shape[0]
    assert cap['t'][ks].tolist() == ts.tolist() and 0 in ts.tolist() and T_LOOP - 1 in ts.tolist()
    t_flat = ts.repeat(B)
    bound = V.term_bounds([v.reshape(-1) for v in ref32], [v.reshape(-1) for v in ref], t_flat)
    got = {key: cap[key][:, ks].reshape(-1) for key in ('vb', 'mse', 'xstart_mse')}
    for k, key in enumerate(('vb', 'mse', 'xstart_mse')):
        err = (got[key] - ref[k].reshape(-1)).abs()
        ratio = err / bound[k]
        w = int(ratio.argmax())
        print(f'[loop vs oracle {net}] {key}: worst error / bound {ratio.max().item():.3f} at t = {int(t_flat[w])} '
              f'(value {ref[k].reshape(-1)[w].item():.4e}, error {err[w].item():.2e}, bound {bound[k][w].item():.2e}); '
              f'worst relative floor of the fp32-fed restatement {V.rel(ref32[k], ref[k]).max().item():.2e}')
    for k, key in enumerate(('vb', 'mse', 'xstart_mse')):
        assert ((got[key] - ref[k].reshape(-1)).abs() <= bound[k]).all(), key
    prior = V.prior(r.x, r.tab)
    assert torch.allclose(cap['prior_bpd'], prior, rtol=8.0 * V.rel(V.prior(r.x, r.tab, V.F32), prior).max().item(), atol=0)


def test_calc_bpd_loop_interface():
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence
    r = rig('c1')
    B = r.shape[0]
    full = r.gd.calc_bpd_loop(r.x, SEED)
    assert _same(full, captured('c1'))
    for key in ('vb', 'mse', 'xstart_mse'):
        assert full[key].shape == (B, T_LOOP) and full[key].dtype == F64 and full[key].device.type == 'cpu'
    assert full['t'].tolist() == list(range(T_LOOP - 1, -1, -1)) and full['prior_bpd'].shape == (B,)
    assert torch.equal(full['total_bpd'], full['prior_bpd'] + full['vb'].sum(1)) and (full['vb'] >= 0).all()
    sub = r.gd.calc_bpd_loop(r.x, SEED, timesteps=10)
    assert sub['total_bpd'] is None and sub['vb'].shape == (B, 10)
    assert sub['t'].tolist() == ddim_time_sequence(T_LOOP, 10)[:-1].tolist()
    assert torch.equal(sub['prior_bpd'], full['prior_bpd'])
    # step k of the subset draws 1 + k: its first level (T - 1, draw 1) is the full run's first column
    assert torch.equal(sub['vb'][:, 0], full['vb'][:, 0])
    noclip = r.gd.calc_bpd_loop(r.x, SEED, timesteps=10, clip_denoised=False)
    assert torch.equal(noclip['mse'], sub['mse']) and not torch.equal(noclip['xstart_mse'], sub['xstart_mse'])


def test_bf16_mode_is_finite_and_near_f32():
    """rmse = sqrt(mse) is a norm of eps_hat - eps, so the two modes' rmse differ by at most rms(eps_hat_bf16 - eps_hat_f32): held to the
    network's own bf16 figure, 2e-2 of rms(eps_hat) (the bound of the bf16 forward against the oracle)."""
    r32, r16 = rig('c1'), rig('c1', 'bf16')
    a, b = r32.run(timesteps=10), r16.run(timesteps=10)
    assert all(torch.isfinite(b[k]).all() for k in ('vb', 'mse', 'xstart_mse', 'prior_bpd'))
    ops = _ops()
    x, tab = r32.x.to(DEV), torch.from_numpy(r32.tab).to(DEV)
    worst = 0.0
    for k, t in enumerate(a['t'].tolist()):
        tt = torch.full((r32.shape[0],), t, dtype=torch.int32, device=DEV)
        eh = r32.unet(ops.vlb_noise(x, tt, tab, seed=SEED, draw=1 + k), tt)
        rms = eh.double().reshape(r32.shape[0], -1).pow(2).mean(1).sqrt().cpu()
        ratio = ((b['mse'][:, k].sqrt() - a['mse'][:, k].sqrt()).abs() / rms).max().item()
        worst = max(worst, ratio)
    print(f'[bf16 vs f32] worst |rmse_bf16 - rmse_f32| / rms(eps_hat) = {worst:.3e} (bound 2e-2)')
    assert worst < 2e-2


# ---- 3. the evaluation's graph lives beside the sampling loops' -------------------------------------------------------------------------

def test_no_eviction_of_the_sampling_graph():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.gaussian_diffusion import vdx_p_sample_loop
    r = rig('c1')
    unet, gd, B = r.unet, r.gd, r.shape[0]
    h = unet.handle(r.shape[2], r.shape[3])
    unet.apply_activation_storage(h)
    ws = unet.workspace(B, r.shape[2], r.shape[3])
    st = torch.cuda.Stream(device=DEV)
    x_T = torch.randn(r.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    img, eps = torch.empty_like(x_T), torch.empty(B, r.shape[2], r.shape[3], r.shape[4], r.shape[1], device=DEV)
    t_dev, step_dev = torch.empty(B, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def steps(n, reset):
        with torch.cuda.stream(st):
            if reset:
                img.copy_(x_T)
                t_dev.fill_(T_LOOP - 1)
                step_dev.zero_()
            with launches() as rec:
                L.check(vdx_p_sample_loop(h.ptr, L.ptr(unet.flat_params), L.ptr(unet.packed()), L.ptr(img), L.ptr(eps), L.ptr(t_dev), L.ptr(step_dev),
                                          L.ptr(gd._ptab), T_LOOP, n, 0, SEED, 1, L.ptr(ws), ws.numel(), B, 1, st.cuda_stream))
            st.synchronize()
        return rec

    first = steps(10, True)                                               # captures: the eager step and the captured one are recorded
    assert sum(k == 'p_sample_kernel' for k, _ in first) == 2
    whole = img.clone()
    assert steps(10, True) == [] and torch.equal(img, whole)              # a replay records nothing
    assert steps(5, True) == []
    with launches() as rec:
        bpd = gd.calc_bpd_loop(r.x, SEED, timesteps=5)
    assert torch.isfinite(bpd['vb']).all() and any(k == 'vlb_term_kernel' for k, _ in rec) and not any(k == 'p_sample_kernel' for k, _ in rec)
    assert steps(5, False) == [], 'the sampling step was captured again: calc_bpd_loop evicted its graph'
    assert torch.equal(img, whole)


def test_sampling_step_is_unchanged_by_the_evaluation():
    """The ancestral step launches what it launched before an evaluation ran on the same handle, and gives the same bits."""
    r = rig('c3')
    with launches() as before:
        a = r.gd.p_sample_loop(r.shape, 11, use_graph=False)
    r.gd.calc_bpd_loop(r.x, SEED, timesteps=3)
    with launches() as after:
        b = r.gd.p_sample_loop(r.shape, 11, use_graph=False)
    assert before == after and torch.equal(a, b)
    assert not any(k.startswith('vlb_') for k, _ in before)


# ---- 4. the command-line tool -----------------------------------------------------------------------------------------------------------

def test_evaluate_cli(tmp_path):
    import yaml
    import evaluate
    cfg = {'unet': dict(dim=16, dim_mults=[1, 2], channels=1, rngs_seed=0, use_bert_text_cond=False),
           'diffusion': dict(image_size=16, num_frames=2, channels=1, timesteps=10, loss_type='l2')}
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    out = tmp_path / 'res' / 'bpd.json'
    evaluate.main(['--random-init', '--config', str(tmp_path / 'cfg.yaml'), '--dataset-path', 'synthetic:4', '--eval-steps', '5', '--batch-size', '3',
                   '--mode', 'f32', '--seed', '4', '--output', str(out)])
    doc = json.loads(out.read_text())
    assert set(doc) == {'total_bpd', 'prior_bpd', 't', 'vb', 'mse', 'xstart_mse', 'num_videos', 'mode', 'seed'}
    assert doc['total_bpd'] is None and doc['num_videos'] == 4 and doc['mode'] == 'f32' and doc['seed'] == 4
    from video_diffusion_nnx_amd.gaussian_diffusion import ddim_time_sequence
    assert doc['t'] == ddim_time_sequence(10, 5)[:-1].tolist()
    for key in ('vb', 'mse', 'xstart_mse'):
        assert len(doc[key]) == 5 and all(np.isfinite(v) for v in doc[key])
    assert np.isfinite(doc['prior_bpd'])
    evaluate.main(['--random-init', '--config', str(tmp_path / 'cfg.yaml'), '--dataset-path', 'synthetic:2', '--mode', 'f32', '--output', str(out)])
    doc = json.loads(out.read_text())
    full = doc
    assert np.isfinite(doc['total_bpd']) and len(doc['t']) == 10 and abs(doc['total_bpd'] - (doc['prior_bpd'] + sum(doc['vb']))) < 1e-9 * abs(doc['total_bpd'])
    assert full['num_videos'] == 2
    # a MovingMNIST file of 0..255 values with --data-scale, and a config the file does not fit
    arr = np.random.default_rng(0).integers(0, 256, (2, 3, 16, 16)).astype(np.uint8)
    np.save(tmp_path / 'mm.npy', arr)
    base = ['--random-init', '--config', str(tmp_path / 'cfg.yaml'), '--mode', 'f32', '--eval-steps', '2', '--output', str(out)]
    evaluate.main(base + ['--dataset-path', str(tmp_path / 'mm.npy'), '--data-scale', '0.00392156862', '--num-videos', '2'])
    doc = json.loads(out.read_text())
    assert doc['num_videos'] == 2 and all(np.isfinite(v) for v in doc['vb'] + doc['mse'] + doc['xstart_mse'])
    cfg['diffusion']['image_size'] = 8
    (tmp_path / 'cfg8.yaml').write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit):
        evaluate.main(['--random-init', '--config', str(tmp_path / 'cfg8.yaml'), '--dataset-path', str(tmp_path / 'mm.npy'), '--output', str(out)])
    # --cond-path: a conditioned network, one row per video; the condition changes the figures; too few rows are refused
    cfg['diffusion']['image_size'] = 16
    cfg['unet']['use_bert_text_cond'] = True
    (tmp_path / 'cfgc.yaml').write_text(yaml.safe_dump(cfg))
    rng = np.random.default_rng(1)
    docs = []
    for k in range(2):
        np.save(tmp_path / f'c{k}.npy', rng.standard_normal((2, 768)).astype(np.float32))
        evaluate.main(['--random-init', '--config', str(tmp_path / 'cfgc.yaml'), '--mode', 'f32', '--eval-steps', '2', '--dataset-path', 'synthetic:2',
                       '--cond-path', str(tmp_path / f'c{k}.npy'), '--output', str(out)])
        docs.append(json.loads(out.read_text()))
    assert all(np.isfinite(v) for d in docs for v in d['mse']) and docs[0]['mse'] != docs[1]['mse']
    with pytest.raises(SystemExit):
        evaluate.main(['--random-init', '--config', str(tmp_path / 'cfgc.yaml'), '--dataset-path', 'synthetic:3', '--cond-path', str(tmp_path / 'c0.npy'),
                       '--output', str(out)])
    with pytest.raises(SystemExit):
        evaluate.main(['--random-init', '--config', str(tmp_path / 'cfg.yaml'), '--dataset-path', 'synthetic:2', '--cond-path', str(tmp_path / 'c0.npy'),
                       '--output', str(out)])
