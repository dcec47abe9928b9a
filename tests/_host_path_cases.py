"""The host paths of gaussian_diffusion.py / train_step.py as cases, shared by tests/test_gpu_host_paths.py and the golden file
tests/golden/host_path_launches.json.  A plain module: nothing here is collected.

run(case) builds the case's own network (a fresh handle: no captured graph is left over from another case), runs it under
tests/_launch_hook.launches() and returns (launches, tensors): the (kernel, shape) pairs in launch order and the CPU copies of what the
path returned.  A sampling case runs three times -- eagerly, captured, and once more -- with a MARK entry in front of each run; the third
run must replay (no forward).  record(case) is the launches alone; encode / decode are the golden file's form of them: every distinct
pair once in a table, a case as indices into it, a block that repeats back to back as [count, block]."""
import tempfile

import torch

from _launch_hook import launches

DEV = 'cuda:0'
T, S, B = 4, 2, 2
SHAPE = (B, 1, 4, 8, 8)                        # C*F*H*W = 256
KW = dict(dim=16, channels=1, dim_mults=(1, 2))
MARK = '--run--'                               # (MARK, 'eager' | 'graph' | 'replay'): where a run of a sampling case starts
SEED = 7


def _gen(seed=5):
    return torch.Generator().manual_seed(seed)


def _gd(kind='plain', **gkw):
    """One fresh (network, diffusion) of the rig: plain | cond | mixed | mixed_cond | sr | lv | focus."""
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.unet3d import Unet3D
    ukw, dkw = dict(KW), dict(gkw)
    if kind in ('cond', 'mixed_cond'):
        ukw['cond_dim'] = 32
    if kind in ('mixed', 'mixed_cond'):
        dkw['frame_noise_alpha'] = 1.0
    if kind == 'sr':
        ukw.update(channels=2, out_dim=1)
        dkw.setdefault('lowres_cond', (2, 2))
    if kind == 'lv':
        ukw['out_dim'] = 2
        dkw['learned_variance'] = True
    if kind == 'focus':
        ukw['focus_present'] = True
    unet = Unet3D(rngs=1, mode='f32', **ukw)
    return GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=T, **dkw)


def _cond():
    return torch.randn(B, 32, generator=_gen(3))


def _video(frames=4):
    return torch.rand(B, 1, frames, 8, 8, generator=_gen(4))


def _lowres():
    return torch.rand(B, 1, 2, 4, 4, generator=_gen(6))


HALF = torch.tensor([1, 1, 0, 0], dtype=torch.bool)

# ---- sampling cases: name -> (kind, diffusion keywords, call(gd, use_graph) -> tensor or tuple of tensors) ----
_LOOPS = {'p': lambda gd, **kw: gd.p_sample_loop(SHAPE, SEED, **kw),
          'ddim': lambda gd, **kw: gd.ddim_sample_loop(SHAPE, SEED, steps=S, **kw),
          'dpm': lambda gd, **kw: gd.dpm_sample_loop(SHAPE, SEED, steps=S, order=2, **kw)}
SAMPLING = {}
for _n, _f in _LOOPS.items():
    SAMPLING[f'{_n}/plain'] = ('plain', {}, lambda gd, g, f=_f: f(gd, use_graph=g))
    SAMPLING[f'{_n}/dyn'] = ('plain', dict(use_dynamic_thres=True), lambda gd, g, f=_f: f(gd, use_graph=g))
    for _phi in (0.0, 0.5):
        SAMPLING[f'{_n}/guided_phi{_phi}'] = ('cond', {}, lambda gd, g, f=_f, phi=_phi: f(gd, use_graph=g, cond=_cond(), cond_scale=2.0,
                                                                                        guidance_rescale=phi))
SAMPLING.update({
    'inpaint/resample1': ('plain', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, resample_steps=1, use_graph=g)),
    'inpaint/resample2': ('plain', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, resample_steps=2, use_graph=g)),
    'inpaint/ddim': ('plain', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, ddim_steps=S, use_graph=g)),
    'inpaint/dpm': ('plain', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, dpm_steps=S, use_graph=g)),
    'inpaint/clean_context': ('plain', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, clean_context=True, use_graph=g)),
    'inpaint/guided': ('cond', {}, lambda gd, g: gd.inpaint(SEED, _video(), HALF, cond=_cond(), cond_scale=2.0, use_graph=g)),
    'extend/two_windows': ('plain', {}, lambda gd, g: gd.extend(SEED, _video(2), 4, context_frames=2, use_graph=g)),
    'mixed/p': ('mixed', {}, lambda gd, g: gd.p_sample_loop(SHAPE, SEED, use_graph=g)),
    'mixed/p_guided': ('mixed_cond', {}, lambda gd, g: gd.p_sample_loop(SHAPE, SEED, cond=_cond(), cond_scale=2.0, use_graph=g)),
    'mixed/ddim': ('mixed', {}, lambda gd, g: gd.ddim_sample_loop(SHAPE, SEED, steps=S, use_graph=g)),
    'sr/p': ('sr', {}, lambda gd, g: gd.upsample(SEED, _lowres(), use_graph=g)),
    'sr/ddim': ('sr', {}, lambda gd, g: gd.upsample(SEED, _lowres(), ddim_steps=S, use_graph=g)),
    'sr/dpm': ('sr', {}, lambda gd, g: gd.upsample(SEED, _lowres(), dpm_steps=S, use_graph=g)),
    'sr/p_aug1': ('sr', {}, lambda gd, g: gd.upsample(SEED, _lowres(), aug_level=1, use_graph=g)),
    'lv/p': ('lv', {}, lambda gd, g: gd.p_sample_loop(SHAPE, SEED, use_graph=g)),
    'lv/p_steps2': ('lv', {}, lambda gd, g: gd.p_sample_loop(SHAPE, SEED, steps=S, use_graph=g)),
    'lv/bpd': ('lv', {}, lambda gd, g: _bpd(gd, g)),
    'plain/bpd': ('plain', {}, lambda gd, g: _bpd(gd, g)),
})


def _bpd(gd, use_graph):
    r = gd.calc_bpd_loop(_video(), SEED, use_graph=use_graph)
    return tuple(r[k] for k in ('vb', 'mse', 'xstart_mse', 'prior_bpd', 'total_bpd'))


def _single(gd, kind):
    """p_sample and p_mean_variance of one diffusion at t = (3, 1)."""
    x = torch.randn(SHAPE, generator=_gen(8))
    t = torch.tensor([3, 1])
    kw = dict(lowres_cond=gd.lowres_condition(_lowres())) if kind == 'sr' else {}
    return (gd.p_sample(x, t, SEED, **kw),) + tuple(gd.p_mean_variance(x, t, True, **kw))


SINGLE = {f'step/{k}': k for k in ('plain', 'mixed', 'sr', 'lv')}

# ---- training cases: name -> (kind, diffusion keywords, trainer attributes, step keywords) ----
TRAINING = {
    'train/l1': ('plain', dict(loss_type='l1'), {}, {}),
    'train/l2': ('plain', dict(loss_type='l2'), {}, {}),
    'train/frame_cond': ('plain', {}, dict(frame_cond_max=2), {}),
    'train/cond_drop': ('cond', {}, dict(null_cond_prob=0.5), dict(cond=True)),
    'train/focus_present': ('focus', {}, dict(prob_focus_present=0.5), {}),
    'train/lv': ('lv', {}, {}, {}),
    'train/tsampler': ('plain', {}, dict(timestep_sampler='loss-second-moment'), {}),
    'train/tsampler_lv': ('lv', {}, dict(timestep_sampler='loss-second-moment'), {}),
    'train/sr_aug': ('sr', dict(lowres_aug_max=2), {}, {}),
    'train/accum2': ('plain', {}, dict(accum=2), {}),
}
CASES = list(SAMPLING) + list(SINGLE) + list(TRAINING)


def _cpu(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    torch.cuda.synchronize()
    return [None if o is None else o.detach().cpu().clone() for o in out]


def _forwards(rec):
    return sum(k.startswith('final_conv') for k, _ in rec)


def _trainer(gd, attrs, tmp):
    """The trainer of tests/test_gpu_grad_controls.py; the switches that Trainer reads in __init__ go on a subclass, the others on the
    instance, so the class defaults stay what they are."""
    from video_diffusion_nnx_amd.trainer import Trainer
    K = attrs.get('accum', 1)
    cls = type('CaseTrainer', (Trainer,), {k: v for k, v in attrs.items() if k == 'timestep_sampler'})
    tr = cls(gd, tmp, dataset_path='synthetic:8', train_batch_size=B, train_num_steps=4, train_lr=1e-3, results_folder=tmp + '/res',
             step_start_ema=0, update_ema_every=1, ema_decay=0.9, gradient_accumulate_every=K, max_grad_norm=None)
    for k, v in attrs.items():
        if k not in ('timestep_sampler', 'accum'):
            setattr(tr, k, v)
    tr.apply_grad_args = K > 1
    return tr


def _train(case):
    """One optimizer step of the case -> (launches, [loss, grads, params], (loss, the p_losses value of the same batch, t and noise))."""
    from video_diffusion_nnx_amd.train_step import run_train_step, run_train_step_accum
    kind, gkw, attrs, skw = TRAINING[case]
    gd = _gd(kind, **gkw)
    unet = gd.denoise_fn
    cond = _cond() if skw.get('cond') else None
    batch = _video()
    with tempfile.TemporaryDirectory() as tmp:
        tr = _trainer(gd, attrs, tmp)
        p0 = unet.flat_params.clone()
        torch.cuda.synchronize()
        with launches() as rec:
            if attrs.get('accum', 1) > 1:
                loss = run_train_step_accum(tr, [batch, _video().flip(0)], 0)
            else:
                loss = run_train_step(tr, batch, 0, **(dict(cond=cond) if cond is not None else {}))
            torch.cuda.synchronize()
        outs = _cpu((loss, tr.grads, unet.flat_params))
        pair = None
        if attrs.get('accum', 1) == 1:
            # the forward value of the same objective on the parameters the step started from
            unet.flat_params.copy_(p0)
            unet.mark_params_updated()
            kw = {}
            if tr.last_frame_mask is not None:
                kw['frame_mask'] = tr.last_frame_mask
            if cond is not None:
                kw.update(cond=cond.to(DEV), cond_mask=None if tr.last_cond_mask is None else tr.last_cond_mask.to(DEV))
            if tr.last_focus_mask is not None:
                kw['focus_present_mask'] = tr.last_focus_mask
            if gd.lowres_cond is not None:
                kw['aug_levels'] = tr.last_aug_levels
                kw['key'] = _loss_key(tr, 0)
            val = gd.p_losses(batch, tr.last_t, noise=gd.noise(SHAPE, tr.last_noise_key, 0), _pre=(2.0, -1.0), **kw)
            pair = (float(loss.item()), float(val.item()))
    return list(rec), outs, pair


def _loss_key(tr, step):
    """The loss key of the step (the key p_losses derives lowres_aug_key from): child 3 of the step key."""
    from video_diffusion_nnx_amd.gaussian_diffusion import split_key
    return split_key(split_key(split_key(tr.rng_seed, tr.rank + 1)[-1], step + 1)[-1], 3)[2]


def run(case):
    """(launches, tensors, extra) of one case; extra: the (train loss, p_losses) pair of a training case, else None."""
    if case in TRAINING:
        return _train(case)
    if case in SINGLE:
        gd = _gd(SINGLE[case])
        torch.cuda.synchronize()
        with launches() as rec:
            out = _single(gd, SINGLE[case])
            torch.cuda.synchronize()
        return list(rec), _cpu(out), None
    kind, gkw, call = SAMPLING[case]
    gd = _gd(kind, **gkw)
    rec_all, outs = [], []
    for what, graph in (('eager', False), ('graph', True), ('replay', True)):
        torch.cuda.synchronize()
        with launches() as rec:
            out = call(gd, graph)
            torch.cuda.synchronize()
        outs += _cpu(out)
        del out
        rec_all += [(MARK, what)] + list(rec)
    return rec_all, outs, None


def record(case):
    return run(case)[0]


def replay_part(rec):
    """The launches of a sampling case's third run."""
    return rec[rec.index((MARK, 'replay')) + 1:]


def forwards(rec):
    return _forwards(rec)


# ---- the golden file's form ----

def _fold(seq):
    """Back-to-back repeats of a block as [count, block], greedily by what the repeat covers."""
    out, i, n = [], 0, len(seq)
    while i < n:
        best_p, best_r = 1, 1
        for p in range(1, (n - i) // 2 + 1):
            r = 1
            while seq[i + r * p:i + (r + 1) * p] == seq[i:i + p]:
                r += 1
            if r > 1 and p * r > best_p * best_r:
                best_p, best_r = p, r
        if best_r > 1:
            out.append([best_r, _fold(seq[i:i + best_p])])
            i += best_p * best_r
        else:
            out.append(seq[i])
            i += 1
    return out


def _unfold(enc):
    out = []
    for e in enc:
        if isinstance(e, list):
            out += _unfold(e[1]) * e[0]
        else:
            out.append(e)
    return out


def encode(records):
    """{case: launches} -> the JSON document."""
    table, index, cases = [], {}, {}
    for case, rec in records.items():
        ids = []
        for pair in rec:
            pair = tuple(pair)
            if pair not in index:
                index[pair] = len(table)
                table.append(list(pair))
            ids.append(index[pair])
        cases[case] = _fold(ids)
    return dict(table=table, cases=cases)


def decode(doc, case):
    return [tuple(doc['table'][i]) for i in _unfold(doc['cases'][case])]
