"""Loss-aware timestep sampling on the GPU (vdx.h: "Loss-aware timestep sampling"): the draw and the update against the fp64
reference of tests/_tsampler_ref.py, the one-pass weighted loss against fp64 sums of the fp32 differences and against vdx_loss_grad's bits,
vdx_hybrid_loss_w against vdx_hybrid_loss and tests/_lv_ref.py, the train step with the sampler on, and two ranks holding one history.

Where the bounds come from: a reordered sum of <= 4096 positive doubles that add up to 1 moves a prefix value by < 4096 * 2^-53 < 5e-13, so
the draw is compared only where every u is farther than 1e-9 from every prefix value of the reference (asserted on the CPU first), and p,
iw and the per-sample losses -- sums of at most 65 553 non-negative doubles in another order -- are held to 1e-12 relative."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lv_ref as R                       # noqa: E402
import _tsampler_ref as TR                # noqa: E402
from _launch_hook import launches        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64


def _dev(t, dtype=None):
    return t.detach().to(dtype or t.dtype).to(DEV).contiguous()


def _ulp32(ref64):
    """Spacing of fp32 at the fp32 rounding of ref64 (towards the larger magnitude), as float64 (tests/test_gpu_learned_variance.py)."""
    r = ref64.float()
    return (torch.nextafter(r.abs(), torch.full_like(r, float('inf'))) - r.abs()).double()


# ---- 1. the draw ------------------------------------------------------------------------------------------------------------------------------

def _history(T, H, seed):
    g = np.random.default_rng(seed)
    return np.exp(g.normal(size=(T, H)) * 2.0)                                  # per-level second moments over several decades


def _raw_draw(hist, count, T, H, eps, batch, key, draw, t_given=None):
    from video_diffusion_nnx_amd import _lib as L, timestep_sampler as TS
    h, c = _dev(torch.from_numpy(hist)), _dev(torch.from_numpy(count))
    t = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    iw = torch.full((batch,), float('nan'), dtype=F64, device=DEV)
    p = torch.full((T,), float('nan'), dtype=F64, device=DEV)
    tg = None if t_given is None else _dev(torch.from_numpy(t_given))
    L.check(TS.vdx_tsampler_draw(L.ptr(h), L.ptr(c), T, H, eps, L.ptr(tg), key, draw, L.ptr(t), L.ptr(iw), L.ptr(p), batch, L.stream_ptr()))
    torch.cuda.synchronize()
    return t.cpu().numpy(), iw.cpu().numpy(), p.cpu().numpy()


@pytest.mark.parametrize('state', ['cold', 'warm', 'given'])
@pytest.mark.parametrize('T,H,B', [(8, 2, 1), (1000, 10, 5), (4096, 32, 300)])
def test_draw_against_reference(T, H, B, state):
    eps, key, drw = 0.001, 0x1234567890ABCDEF + T, 3 if T == 1000 else 0
    ref = TR.RefSampler(T, H, eps)
    count = np.full(T, H, dtype=np.int32)
    if state == 'cold':
        count[T // 2] = H - 1
    ref.load_state(_history(T, H, T + H), count)
    t_given = None
    if state == 'given':
        t_given = (np.random.default_rng(B).integers(0, T, size=B)).astype(np.int32)
        t_given[0] = T - 1
    else:
        u, cum = ref.uniforms(B, key, drw), (ref.prefix() if state == 'warm' else np.arange(1, T + 1) / T)
        margin = np.abs(u[:, None] - cum[None, :]).min()
        assert margin > 1e-9, f'pick another key: a u is {margin:.2e} from a prefix value'
    t_ref, iw_ref = ref.draw(B, key, drw, t=t_given)
    p_ref = ref.probabilities()
    got = [_raw_draw(ref.hist, ref.count, T, H, eps, B, key, drw, t_given) for _ in range(2)]
    for a, b in zip(*got):
        assert np.array_equal(a, b), 'two calls are not bit-identical'
    t, iw, p = got[0]
    assert np.array_equal(t, t_ref), (t, t_ref)
    assert np.all(np.abs(p - p_ref) <= 1e-12 * p_ref) and np.all(np.abs(iw - iw_ref) <= 1e-12 * iw_ref)
    if state == 'cold':
        assert np.array_equal(iw, np.ones(B)) and np.array_equal(p, np.full(T, 1.0 / T))
    else:
        assert abs(p.sum() - 1.0) < 1e-12 and (iw != 1.0).any()
    if state == 'warm' and B > 1:
        assert len(set(t.tolist())) > 1
    # the Python wrapper is this call
    from video_diffusion_nnx_amd.timestep_sampler import LossSecondMomentSampler
    s = LossSecondMomentSampler(T, H, eps, device=DEV)
    s.load_state(torch.from_numpy(ref.hist), torch.from_numpy(ref.count))
    t2, iw2 = s.draw(B, key, drw, t=None if t_given is None else torch.from_numpy(t_given))
    assert np.array_equal(t2.cpu().numpy(), t) and np.array_equal(iw2.cpu().numpy(), iw) and np.array_equal(s.probabilities().cpu().numpy(), p)
    assert s.warm == (state != 'cold')


# ---- 2. the update ----------------------------------------------------------------------------------------------------------------------------

def test_update_against_reference_bit_for_bit():
    from video_diffusion_nnx_amd.timestep_sampler import LossSecondMomentSampler
    T, H, n = 8, 3, 300
    g = np.random.default_rng(4)
    e = np.stack([g.integers(0, 7, size=n).astype(np.float64), np.exp(g.normal(size=n))], 1)
    e[5:9, 0] = 2.0                                                              # repeats of one level, side by side
    e[[40, 250], 0] = 7.0                                                        # level 7 is seen twice: its row stays at H - 1
    e[100] = (3.0, float('nan'))                                                 # three bad entries, skipped
    e[101] = (3.0, float('inf'))
    e[102] = (8.0, 1.0)
    ref = TR.RefSampler(T, H)
    s = LossSecondMomentSampler(T, H, device=DEV)
    e[:4, 0] = 5.0                                                               # row 5 goes H - 1 -> H -> shift over the first three calls
    for lo, hi in ((0, 2), (2, 3), (3, 4), (4, n)):
        ref.update(e[lo:hi])
        with launches() as rec:
            s.update(torch.from_numpy(e[lo:hi]))
        assert [k for k, _ in rec] == ['tsampler_update_kernel']
        hist, count = s.state()
        assert np.array_equal(count.cpu().numpy(), ref.count), (lo, hi)
        assert np.array_equal(hist.cpu().numpy().view(np.uint64), ref.hist.view(np.uint64)), (lo, hi)
    assert ref.count.tolist() == [3] * 7 + [2] and not s.warm


# ---- 3. vdx_loss_weighted -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('l2', [False, True], ids=['l1', 'l2'])
@pytest.mark.parametrize('B,C,fhw', [(1, 1, 35), (3, 3, 21), (2, 3, 21851), (2, 2, 32)])       # (the last: whole quads, the float4 loads)
def test_loss_weighted(B, C, fhw, l2):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd.timestep_sampler import loss_weighted
    from video_diffusion_nnx_amd.train_step import vdx_loss_grad
    g = torch.Generator().manual_seed(B * 100 + C)
    noise = torch.randn(B, C, 1, 1, fhw, generator=g)
    eh = noise + 0.5 * torch.randn(B, C, 1, 1, fhw, generator=g)
    eh.view(-1)[1] = noise.view(-1)[1]                                           # d = 0: the sign is 0
    iw = torch.rand(B, generator=g, dtype=F64) * 4.8 + 0.2
    eh_cl = eh.permute(0, 2, 3, 4, 1).contiguous()                               # channel-last, as the network writes it
    d = eh - noise                                                               # fp32, as the kernels form it
    el = d.double() ** 2 if l2 else d.double().abs()
    l_ref = el.reshape(B, -1).mean(1)
    n = B * C * fhw
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(n), dtype=F32)

    def grad_ref(w):
        f = (w.float() * inv).reshape(B, 1, 1, 1, 1)
        return ((2.0 * d * f) if l2 else (torch.sign(d) * f)).permute(0, 2, 3, 4, 1).contiguous()
    ehd, nd = _dev(eh_cl), _dev(noise)
    plain = torch.empty_like(ehd)
    L.check(vdx_loss_grad(L.ptr(ehd), L.ptr(nd), L.ptr(plain), B, C, fhw, int(l2), L.stream_ptr()))
    for name, w in (('iw', iw), ('ones', torch.ones(B, dtype=F64)), ('null', None)):
        with launches() as rec:
            out, d_eps = loss_weighted(ehd, nd, None if w is None else _dev(w), l2=l2)
        torch.cuda.synchronize()
        assert [k for k, _ in rec] == ['loss_weighted_kernel', 'loss_weighted_final_kernel']
        out = out.cpu()
        wv = torch.ones(B, dtype=F64) if w is None else w
        err = ((out[:B] - l_ref).abs() / l_ref).max().item()
        tot_ref = (wv * l_ref).mean()
        print(f'[loss_weighted {B}x{C}x{fhw} l2={int(l2)} {name}] per-sample rel err {err:.2e}, total rel err '
              f'{abs(out[B] - tot_ref).item() / tot_ref.item():.2e} (bound 1e-12)')
        assert err <= 1e-12 and abs(out[B] - tot_ref).item() <= 1e-12 * tot_ref.item()
        assert torch.equal(d_eps.cpu(), grad_ref(wv)), f'{name}: d_eps is not the stated fp32 expression bit for bit'
        if w is None or name == 'ones':
            assert torch.equal(d_eps, plain), f'{name}: d_eps is not vdx_loss_grad bit for bit'
        else:
            assert not torch.equal(d_eps, plain)
        out2, none = loss_weighted(ehd, nd, None if w is None else _dev(w), l2=l2, want_grad=False)
        assert none is None and torch.equal(out2.cpu(), out)


# ---- 4. vdx_hybrid_loss_w -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _hybrid_ref(name, l2, w):
    c = R.hybrid_case(name)
    tab = R.tables()['tab64']
    vals, grad = R.hybrid_grad(c['x0'], c['eps'], c['out2'], c['t'], tab, l2, w)
    with torch.no_grad():
        v32 = R.hybrid(c['x0'], c['eps'], c['out2'], c['t'], tab, l2, w, dt=F32)
    return vals, grad, {k: u.double() for k, u in v32.items()}


@pytest.mark.parametrize('l2', [False, True], ids=['l1', 'l2'])
def test_hybrid_loss_w(l2, name='C3_ODD'):
    """The smallest case of tests/test_gpu_learned_variance.py (per_sample 210, t = (0, 1, T - 1, random))."""
    from video_diffusion_nnx_amd import ops
    c = R.hybrid_case(name)
    assert 0 in c['t'].tolist()
    B, C = c['shape'][0], c['shape'][1]
    w = 0.37
    vals, g_ref, v32 = _hybrid_ref(name, l2, w)
    tab = _dev(torch.from_numpy(R.tables()['tab64']))
    x, eps, out2, t = _dev(c['x0']), _dev(c['eps']), _dev(c['out2']), _dev(c['t'])
    base, base_g = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=True)
    null, null_g = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=True, weighted=True)
    torch.cuda.synchronize()
    assert torch.equal(null, base) and torch.equal(null_g, base_g), 'iw = NULL is not vdx_hybrid_loss bit for bit'
    one, one_g = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=True, iw=torch.ones(B, dtype=F64, device=DEV))
    assert torch.equal(one, base) and torch.equal(one_g, base_g), 'iw = 1 is not vdx_hybrid_loss bit for bit'
    g = torch.Generator().manual_seed(11)
    iw = torch.rand(B, generator=g, dtype=F64) * 4.8 + 0.2
    runs = []
    for _ in range(2):
        out, d_out = ops.hybrid_loss(x, eps, out2, t, tab, l2=l2, vlb_weight=w, want_grad=True, iw=_dev(iw))
        torch.cuda.synchronize()
        runs.append((out.cpu(), d_out.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'two runs are not bit-identical'
    out, d_out = runs[0]
    assert torch.equal(out[:2 * B], base.cpu()[:2 * B]), 'the per-sample pairs must stay unweighted'
    # the totals: the bound tests/test_gpu_learned_variance.py holds the unweighted totals to, on the weighted sums of the same references
    loss_b = lambda v: v['mse_b'] + w * v['vb_b']
    for i, (key, f) in enumerate((('mse', lambda v: v['mse_b']), ('vb', lambda v: v['vb_b']), ('loss', loss_b))):
        ref, ref32 = (iw * f(vals)).mean().item(), (iw * f(v32)).mean().item()
        tol = 8.0 * max(abs(ref32 - ref), 2.0 ** -52 * abs(ref))
        err = abs(out[2 * B + i].item() - ref)
        print(f'[hybrid_w {name} l2={int(l2)}] {key}: {out[2 * B + i].item():.12g} ref {ref:.12g} |err| {err:.2e} bound {tol:.2e}')
        assert err <= tol
    # the gradient: within 1 fp32 ulp of the fp64 gradient times iw_b, both halves
    want = g_ref * iw.reshape(B, 1, 1, 1, 1)
    ulps = ((d_out.double() - want).abs() / _ulp32(want)).max().item()
    print(f'[hybrid_w {name} l2={int(l2)}] d_out: worst |got - fp64 * iw| = {ulps:.3f} fp32 ulp (bound 1)')
    assert ulps <= 1.0
    assert not torch.equal(d_out, base_g.cpu())


# ---- 5. the train step --------------------------------------------------------------------------------------------------------------------------

TRAIN_KW = dict(dim=16, dim_mults=(1, 2), channels=1)                            # tests/test_gpu_learned_variance.py's TRAIN_KW-sized network
TRAIN_SHAPE = (2, 1, 2, 16, 16)
T_TRAIN = 8


def _mk(tmp_path, monkeypatch, sampler, lv=False, H=10):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    monkeypatch.setattr(Trainer, 'timestep_sampler', 'loss-second-moment' if sampler else 'uniform')
    monkeypatch.setattr(Trainer, 'sampler_history', H)
    unet = Unet3D(rngs=1, mode='f32', **dict(TRAIN_KW, out_dim=2 if lv else None))
    gd = GaussianDiffusion(unet, image_size=16, num_frames=2, channels=1, timesteps=T_TRAIN, loss_type='l2', learned_variance=lv)
    tr = Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=8, train_lr=1e-3,
                 checkpoint_every_steps=100, results_folder=str(tmp_path / 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9)
    return unet, gd, tr


def _entries(tr):
    return np.stack([tr.last_t.cpu().numpy().astype(np.float64), tr.last_loss_per_sample.cpu().numpy()], 1)


@pytest.mark.parametrize('lv', [False, True], ids=['plain', 'learned_variance'])
def test_train_step_cold_is_the_uniform_step_at_the_same_t(tmp_path, monkeypatch, lv):
    from video_diffusion_nnx_amd import train_step as S
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(*TRAIN_SHAPE, generator=g)
    _, _, on = _mk(tmp_path / 'on', monkeypatch, True, lv)
    with launches() as rec:
        loss_on = on.train_step(batch, step=0)
    torch.cuda.synchronize()
    names = [k for k, _ in rec]
    assert names.count('tsampler_draw_kernel') == 1 and names.count('tsampler_update_kernel') == 1
    assert ('hybrid_loss_kernel' in names) == lv and ('loss_weighted_kernel' in names) == (not lv)
    assert 'loss_kernel' not in names and 'loss_grad_kernel' not in names
    # the update is enqueued behind the backward: the last launch before the optimizer
    assert names.index('tsampler_draw_kernel') < names.index('tsampler_update_kernel') == names.index('adam_ema_kernel') - 1
    assert on.last_t.device.type == 'cuda' and on.last_iw.dtype == F64 and on.last_loss_per_sample.dtype == F64
    assert torch.equal(on.last_iw.cpu(), torch.ones(2, dtype=F64))
    # the draw is the reference's, under micro_step_keys' t_key, draw 0
    ref = TR.RefSampler(T_TRAIN, 10)
    t_ref, _ = ref.draw(2, S.micro_step_keys(on.rng_seed, on.rank, 0)[0], 0)
    assert np.array_equal(on.last_t.cpu().numpy(), t_ref)
    grads_on = on.grads.clone()
    _, _, off = _mk(tmp_path / 'off', monkeypatch, False, lv)
    assert off.sampler is None
    loss_off = off.train_step(batch, step=0, t=on.last_t)
    torch.cuda.synchronize()
    assert torch.equal(off.grads, grads_on), 'cold sampler: the gradient is not the uniform step\'s bit for bit'
    assert grads_on.abs().max() > 0
    print(f'[train cold lv={int(lv)}] loss on {loss_on.item():.8f} off {loss_off.item():.8f}')
    assert abs(loss_on.item() - loss_off.item()) <= 1e-6 * abs(loss_off.item())
    # after the step the history holds (t_b, l_b)
    ref.update(_entries(on))
    hist, count = on.sampler.state()
    assert np.array_equal(count.cpu().numpy(), ref.count) and np.array_equal(hist.cpu().numpy().view(np.uint64), ref.hist.view(np.uint64))
    assert ref.count.sum() == 2


@pytest.mark.parametrize('lv', [False, True], ids=['plain', 'learned_variance'])
def test_six_warm_steps_follow_the_reference(tmp_path, monkeypatch, lv):
    from video_diffusion_nnx_amd import train_step as S
    H = 2
    _, _, tr = _mk(tmp_path, monkeypatch, True, lv, H=H)
    hist0 = _history(T_TRAIN, H, 17)
    count0 = np.full(T_TRAIN, H, dtype=np.int32)
    tr.sampler.load_state(torch.from_numpy(hist0), torch.from_numpy(count0))
    ref = TR.RefSampler(T_TRAIN, H, tr.sampler.uniform_prob)
    ref.load_state(hist0, count0)
    g = torch.Generator().manual_seed(0)
    seen = set()
    for step in range(6):
        t_ref, iw_ref = ref.draw(2, S.micro_step_keys(tr.rng_seed, tr.rank, step)[0], 0)
        loss = tr.train_step(torch.rand(*TRAIN_SHAPE, generator=g), step=step)
        torch.cuda.synchronize()
        t, iw = tr.last_t.cpu().numpy(), tr.last_iw.cpu().numpy()
        assert np.array_equal(t, t_ref), (step, t, t_ref)
        assert np.all(np.abs(iw - iw_ref) <= 1e-12 * iw_ref), (step, iw, iw_ref)
        lb = tr.last_loss_per_sample.cpu().numpy()
        assert np.isfinite(lb).all() and abs(loss.item() - float(np.mean(iw * lb))) <= 1e-6 * abs(loss.item())      # the weighted mean
        ref.update(_entries(tr))                                                 # the device's own recorded losses
        seen.update(t.tolist())
    hist, count = tr.sampler.state()
    assert np.array_equal(count.cpu().numpy(), ref.count) and np.array_equal(hist.cpu().numpy().view(np.uint64), ref.hist.view(np.uint64))
    assert not np.array_equal(ref.hist, hist0) and len(seen) > 1 and tr.opt_count == 6
    assert torch.isfinite(tr.unet.flat_params).all()


def test_frame_mask_raises(tmp_path, monkeypatch):
    _, _, tr = _mk(tmp_path, monkeypatch, True)
    with launches() as rec:
        with pytest.raises(ValueError, match='frame'):
            tr.train_step(torch.rand(*TRAIN_SHAPE), step=0, frame_mask=torch.tensor([1, 0]))
    assert rec == []


# ---- 6. two ranks on one GPU --------------------------------------------------------------------------------------------------------------------

def _rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    sys.path.insert(0, ROOT)
    import tempfile
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
        from video_diffusion_nnx_amd.trainer import Trainer
        from video_diffusion_nnx_amd.unet3d import Unet3D
        Trainer.timestep_sampler, Trainer.sampler_history, Trainer.min_bucket_floats = 'loss-second-moment', 2, 1 << 12
        unet = Unet3D(rngs=1, mode='f32', **TRAIN_KW)
        gd = GaussianDiffusion(unet, image_size=16, num_frames=2, channels=1, timesteps=T_TRAIN, loss_type='l2')
        tmp = tempfile.mkdtemp()
        tr = Trainer(gd, tmp, dataset_path='synthetic:8', train_batch_size=4, train_num_steps=2, train_lr=1e-3, results_folder=tmp)
        assert tr.world == world and tr.per_device_bs == 2
        g = torch.Generator().manual_seed(5)
        entries = []
        for s in range(2):
            x = torch.rand(4, *TRAIN_SHAPE[1:], generator=g)
            tr.train_step(x[2 * rank:2 * rank + 2], s)
            torch.cuda.synchronize()
            entries.append(_entries(tr))
        hist, count = tr.sampler.state()
        refused = False
        Trainer.comm_backend = 'abi'
        try:
            Trainer(gd, tmp, dataset_path='synthetic:8', train_batch_size=4, train_num_steps=2, results_folder=tmp)
        except ValueError as e:
            refused = 'gather' in str(e)
        q.put((rank, (hist.cpu().numpy(), count.cpu().numpy(), entries, refused)))       # numpy: pickled by value through the mp queue
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_one_history():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29300 + os.getpid() % 200
    ps = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    outs = dict(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(60)
    (ha, ca, ea, ra), (hb, cb, eb, rb) = outs[0], outs[1]
    assert np.array_equal(ha.view(np.uint64), hb.view(np.uint64)) and np.array_equal(ca, cb), 'the ranks hold different histories'
    ref = TR.RefSampler(T_TRAIN, 2)
    for s in range(2):
        ref.update(np.concatenate([ea[s], eb[s]], 0))                            # (rank, sample) order
    assert np.array_equal(ca, ref.count) and np.array_equal(ha.view(np.uint64), ref.hist.view(np.uint64))
    assert ref.count.sum() >= 4 and not np.array_equal(ea[0], eb[0])
    assert ra and rb, "comm_backend='abi' with two ranks must raise"
