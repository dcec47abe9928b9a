"""Gradient accumulation and global-norm clipping behind Trainer.apply_grad_args (the reference documents gradient_accumulate_every and
max_grad_norm, marks the first TODO and never calls its clip_grad_norm, utils.py:127-152):

  kernels      vdx_grad_accumulate (bit-exact adds at every alignment, neighbours untouched), vdx_grad_sqnorm (double, reproducible,
               alignment-independent), vdx_adam_ema_step_clip (clip == 1: vdx_adam_ema_step's bits; clip < 1: the fp64 restatement);
  train step   K micro-batches == one large batch, the switch without effect at K = 1 / no clipping, the clip as the trainer applies
               it, run-to-run bits, and two ranks x K = 2 against one rank on the global batch.

The network is the tiny one of tests/test_gpu_train.py (dim 16, dim_mults (1, 2), 4 frames, 8 x 8)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS = [1, 5, 255, 1027, (1 << 20) + 7]
OFFSETS = [(0, 0), (1, 1), (3, 2)]                     # (acc, g) offsets in floats into larger (256-byte aligned) buffers
PAD = 8

# fp64 oracle gradient norm of _inputs() on the Unet3D(rngs=1) initialisation (oracle/train_ref.loss_and_grads over
# oracle/diffusion_ref + oracle/unet3d_ref, mean l2 loss of the batch of 4): 16.6956.  MAX_NORM is below half of it, so the clip is active.
ORACLE_NORM = 16.6956
MAX_NORM = 4.0


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------ kernels ------------------------------------------------------------------

@pytest.mark.parametrize('offs', OFFSETS)
@pytest.mark.parametrize('n', NS)
def test_grad_accumulate_bit_exact(n, offs):
    from video_diffusion_nnx_amd import ops
    oa, og = offs
    g = torch.Generator().manual_seed(n + 7 * oa + og)
    A = torch.randn(n + 2 * PAD, generator=g)
    G = torch.randn(n + 2 * PAD, generator=g)
    exp = A.clone()
    exp[oa:oa + n] = A[oa:oa + n] + G[og:og + n]           # one fp32 add per element: no reordering, the same bits on any device
    dA, dG = A.cuda(), G.cuda()
    ops.grad_accumulate(dA[oa:oa + n], dG[og:og + n])
    torch.cuda.synchronize()
    assert torch.equal(dA.cpu(), exp), 'acc + g differs, or a float outside [0, n) was written'
    assert torch.equal(dG.cpu(), G)


@pytest.mark.parametrize('n', NS)
def test_grad_sqnorm_matches_fp64_and_is_reproducible(n):
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    ref = (x.double() ** 2).sum().item()
    bits = []
    for og in sorted({o for _, o in OFFSETS}):
        buf = torch.zeros(n + 2 * PAD)
        buf[og:og + n] = x
        d = buf.cuda()
        a = ops.grad_sqnorm(d[og:og + n]).cpu()
        b = ops.grad_sqnorm(d[og:og + n]).cpu()
        rel = abs(a.item() - ref) / ref
        print(f'[sqnorm n={n} offset={og}] rel {rel:.3e}')
        assert rel <= 1e-10, rel
        assert torch.equal(a, b), 'two calls on the same data differ'
        bits.append(a)
    assert all(torch.equal(bits[0], b) for b in bits[1:]), 'the result depends on the alignment of g'


def test_grad_sqnorm_squares_in_double():
    """Magnitudes whose float square underflows (1e-25 -> 1e-50) or dominates a float sum (1e15 -> 1e30)."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(3)
    tiny = torch.randn(1027, generator=g) * 1e-25
    ref = (tiny.double() ** 2).sum().item()
    assert (tiny * tiny).sum().item() == 0.0 and ref > 0
    got = ops.grad_sqnorm(tiny.cuda()).item()
    print(f'[sqnorm 1e-25] {got:.6e} vs {ref:.6e}')
    assert abs(got - ref) / ref <= 1e-10
    mixed = torch.randn(1027, generator=g)
    mixed[5::97] = 1e-25
    mixed[11::201] = 1e15
    mixed[1026] = -1e15
    ref = (mixed.double() ** 2).sum().item()
    got = ops.grad_sqnorm(mixed.cuda()).item()
    print(f'[sqnorm mixed] {got:.17e} vs {ref:.17e}')
    assert abs(got - ref) / ref <= 1e-10


def _adam_inputs(n=10007):
    g = torch.Generator().manual_seed(17)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    m = 0.05 * torch.randn(n, generator=g)                 # non-zero moments: from zero, Adam's first step is lr * sign(g) and hides any scale
    v = 1e-3 * (0.5 + torch.rand(n, generator=g))
    ema = p + 0.01 * torch.randn(n, generator=g)
    return p, grad, m, v, ema


HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step_count=3, grad_scale=0.5, do_ema=True, ema_decay=0.9)


def test_adam_clip_kernel_without_clip_is_adam_ema_step():
    from video_diffusion_nnx_amd import ops
    host = _adam_inputs()
    a = [t.cuda() for t in host]
    b = [t.cuda() for t in host]
    ops.adam_ema_step(*a, **HYP)
    norm = ops.adam_ema_step_clip(*b, ops.grad_sqnorm(b[1]), 1e30, **HYP)
    torch.cuda.synchronize()
    for name, x, y in zip(('p', 'g', 'm', 'v', 'ema'), a, b):
        assert torch.equal(x, y), f'{name}: clip == 1 must leave the bits of vdx_adam_ema_step'
    ref = torch.sqrt((0.5 * host[1].double()).pow(2).sum() + 1e-6).item()
    assert abs(norm.item() - ref) / ref <= 1e-6


def _adam_restated(p, grad, m, v, ema, max_norm):
    """utils.clip_grad_norm of the averaged gradient, then oracle/train_ref.adam_update and the EMA, in the dtype of the inputs."""
    from oracle import train_ref
    from video_diffusion_nnx_amd.utils import clip_grad_norm
    gs = grad * HYP['grad_scale']
    l2 = torch.sqrt((gs.double() ** 2).sum() + 1e-6)
    if max_norm is not None:
        gs, l2 = clip_grad_norm(gs, max_norm)
    p1, m1, v1 = train_ref.adam_update({'p': p}, {'p': gs}, {'p': m}, {'p': v}, count=HYP['step_count'], lr=HYP['lr'],
                                       b1=HYP['b1'], b2=HYP['b2'], eps=HYP['eps'])
    e1 = HYP['ema_decay'] * ema + (1 - HYP['ema_decay']) * p1['p']
    return dict(p=p1['p'], m=m1['p'], v=v1['p'], ema=e1, norm=l2.to(p.dtype).reshape(1))


def test_adam_clip_kernel_matches_fp64_restatement():
    """max_grad_norm = 1 against ||0.5 g|| ~ 50: clip ~ 0.02.  Bound per tensor: 8 x the rel-L2 error of the same formulas evaluated in
    fp32 on the CPU against the fp64 result; the UNclipped fp64 m and v must violate it, so a missing clip cannot pass."""
    from video_diffusion_nnx_amd import ops
    host = _adam_inputs()
    ref = _adam_restated(*[t.double() for t in host], 1.0)
    f32 = _adam_restated(*host, 1.0)
    unclipped = _adam_restated(*[t.double() for t in host], None)
    d = [t.cuda() for t in host]
    norm = ops.adam_ema_step_clip(*d, ops.grad_sqnorm(d[1]), 1.0, **HYP)
    torch.cuda.synchronize()
    got = dict(p=d[0], m=d[2], v=d[3], ema=d[4], norm=norm)
    assert 40.0 < ref['norm'].item() < 60.0
    fails = []
    for k in ('p', 'm', 'v', 'ema', 'norm'):
        e32, e = _rel(f32[k], ref[k]), _rel(got[k], ref[k])
        print(f'[adam clip {k}] fp32-on-CPU rel {e32:.3e}  bound {8 * e32:.3e}  kernel rel {e:.3e}')
        if not e <= 8 * e32:
            fails.append((k, e, 8 * e32))
        if k in ('m', 'v'):
            eu = _rel(unclipped[k], ref[k])
            print(f'[adam clip {k}] unclipped fp64 rel {eu:.3e}')
            assert eu > 8 * e32, f'{k}: the bound does not tell a missing clip apart'
    assert not fails, fails
    assert torch.equal(d[1].cpu(), host[1]), 'the gradient buffer is read-only'


# ---------------------------------------------------------------- train step ----------------------------------------------------------------

def _mk(tmp, mode='f32', on=True, K=1, max_norm=None, batch=2, seed_unet=1):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(rngs=seed_unet, mode=mode, dim=16, channels=1, dim_mults=(1, 2))
    gd = GaussianDiffusion(unet, image_size=8, num_frames=4, channels=1, timesteps=50, loss_type='l2')
    tr = Trainer(gd, str(tmp), dataset_path='synthetic:8', train_batch_size=batch, train_num_steps=4, train_lr=1e-3,
                 results_folder=os.path.join(str(tmp), 'res'), step_start_ema=0, update_ema_every=1, ema_decay=0.9,
                 gradient_accumulate_every=K, max_grad_norm=max_norm)
    tr.apply_grad_args = on                                    # on the instance: the class default stays False for every other test
    return unet, tr


def _inputs():
    """The global batch of 4 whose oracle gradient norm is ORACLE_NORM."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 1, 4, 8, 8, generator=g)
    t = torch.randint(0, 50, (4,), generator=g)
    noise = torch.randn(4, 1, 4, 8, 8, generator=g)
    return x, t, noise


def _state(unet, tr):
    torch.cuda.synchronize()
    return dict(p=unet.flat_params.clone(), m=tr.m.clone(), v=tr.v.clone(), ema=tr.ema.clone(), g=tr.grads.clone())


def test_accumulation_equals_large_batch(tmp_path):
    x, t, noise = _inputs()
    ua, A = _mk(tmp_path / 'a', on=True, K=2)
    la = A.train_step_accum([x[:2], x[2:]], 0, ts=[t[:2], t[2:]], noises=[noise[:2], noise[2:]])
    ub, B = _mk(tmp_path / 'b', on=False)
    lb = B.train_step(x, 0, t=t, noise=noise)
    torch.cuda.synchronize()
    assert B.micro_grads is None and A.micro_grads is not None
    rel = _rel(A.grads / 2, B.grads)
    print(f'[accum K=2 vs batch 4] grads rel-L2 {rel:.3e}  loss {la.item():.7f} vs {lb.item():.7f}')
    assert rel <= 2e-5, rel
    assert abs(la.item() - lb.item()) <= 1e-5 * abs(lb.item())
    assert A.opt_count == 1 and B.opt_count == 1
    assert A.last_grad_norm is None                            # no clipping, no norm asked for: the plain optimizer kernel ran


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_switch_is_inert_at_k1_without_clipping(tmp_path, mode):
    ends = []
    for on in (True, False):
        unet, tr = _mk(tmp_path / f'on{int(on)}', mode=mode, on=on, K=1, max_norm=None)
        g = torch.Generator().manual_seed(5)
        for step in range(2):
            batch = torch.rand(2, 1, 4, 8, 8, generator=g)
            loss = tr.train_step_accum([batch], step) if on else tr.train_step(batch, step)
        ends.append((_state(unet, tr), loss.item()))
        assert tr.micro_grads is None and tr.last_grad_norm is None and tr.opt_count == 2
    for k in ('p', 'm', 'v', 'ema'):
        assert torch.equal(ends[0][0][k], ends[1][0][k]), k
    assert ends[0][1] == ends[1][1]


def test_trainer_clips_to_max_grad_norm(tmp_path):
    x, t, noise = _inputs()
    unet, tr = _mk(tmp_path, on=True, K=1, max_norm=MAX_NORM, batch=4)
    tr.train_step_accum([x], 0, ts=[t], noises=[noise])
    torch.cuda.synchronize()
    norm = tr.last_grad_norm.item()
    print(f'[trainer clip] last_grad_norm {norm:.6f} (fp64 oracle {ORACLE_NORM}), max_grad_norm {MAX_NORM}')
    assert norm >= 2 * MAX_NORM
    assert abs(norm - ORACLE_NORM) <= 1e-3 * ORACLE_NORM
    g64 = tr.grads.cpu().double()
    l2 = torch.sqrt((g64 ** 2).sum() + 1e-6).item()
    assert abs(norm - l2) / l2 <= 1e-6
    clip = min(MAX_NORM / (l2 + 1e-6), 1.0)
    rel = _rel(tr.m, 0.1 * clip * g64)
    print(f'[trainer clip] clip {clip:.6f}  m vs 0.1 * clip * grads rel-L2 {rel:.3e}')
    assert rel <= 1e-6, rel
    assert tr.opt_count == 1


def test_norm_without_clipping_leaves_the_step_unchanged(tmp_path):
    """Trainer.track_grad_norm without max_grad_norm: the clipping kernel at FLT_MAX -- the norm is reported, the step keeps its bits."""
    x, t, noise = _inputs()
    ends = []
    for track in (True, False):
        unet, tr = _mk(tmp_path / f't{int(track)}', on=True, K=1, max_norm=None, batch=4)
        tr.track_grad_norm = track
        tr.train_step_accum([x], 0, ts=[t], noises=[noise])
        ends.append((_state(unet, tr), tr.last_grad_norm))
    for k in ends[0][0]:
        assert torch.equal(ends[0][0][k], ends[1][0][k]), k
    l2 = torch.sqrt((ends[0][0]['g'].cpu().double() ** 2).sum() + 1e-6).item()
    assert ends[1][1] is None and abs(ends[0][1].item() - l2) / l2 <= 1e-6


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_accumulated_clipped_steps_are_bit_reproducible(tmp_path, mode):
    ends = []
    for run in range(2):
        unet, tr = _mk(tmp_path / f'r{run}', mode=mode, on=True, K=2, max_norm=MAX_NORM)
        g = torch.Generator().manual_seed(5)
        losses = []
        for step in range(2):
            batches = [torch.rand(2, 1, 4, 8, 8, generator=g) for _ in range(2)]
            losses.append(tr.train_step_accum(batches, step).item())       # the trainer's own t / noise draws per micro-step
        st = _state(unet, tr)
        st['norm'] = tr.last_grad_norm.clone()
        ends.append((st, losses))
        assert tr.opt_count == 2
    assert ends[0][1] == ends[1][1], (ends[0][1], ends[1][1])
    for k in ends[0][0]:
        assert torch.equal(ends[0][0][k], ends[1][0][k]), k


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        q.put((rank, _rank_step(world, rank)))
    finally:
        dist.destroy_process_group()


def _rank_step(world, rank):
    """world ranks x K micro-batches of the global batch of 4, one sample each (world 2, K 2), or one rank on all 4 (world 1, K 1)."""
    import tempfile
    from video_diffusion_nnx_amd.trainer import Trainer
    x, t, noise = _inputs()
    K = 2 if world == 2 else 1
    per = 4 // (world * K)
    Trainer.min_bucket_floats = 1 << 12                       # several buckets on this small network (this process only, when spawned)
    unet, tr = _mk(tempfile.mkdtemp(), on=True, K=K, max_norm=MAX_NORM, batch=per * world)
    assert tr.world == world and tr.per_device_bs == per and len(tr.buckets) >= 2
    sl = [slice((rank * K + j) * per, (rank * K + j + 1) * per) for j in range(K)]
    loss = tr.train_step_accum([x[s] for s in sl], 0, ts=[t[s] for s in sl], noises=[noise[s] for s in sl])
    torch.cuda.synchronize()
    assert tr.opt_count == 1
    return unet.flat_params.cpu().numpy(), tr.m.cpu().numpy(), float(tr.last_grad_norm.item()), float(loss.item())


def test_two_ranks_accumulating_match_one_rank_on_global_batch():
    import torch.multiprocessing as mp
    from video_diffusion_nnx_amd.trainer import Trainer
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29300 + os.getpid() % 200
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    outs = dict(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(60)
    keep = Trainer.min_bucket_floats
    try:
        p1, m1, n1, l1 = _rank_step(1, 0)
    finally:
        Trainer.min_bucket_floats = keep
    (pa, ma, na, la), (pb, mb, nb, lb) = outs[0], outs[1]
    assert np.array_equal(pa, pb) and np.array_equal(ma, mb) and na == nb, 'the replicas diverged'
    assert na >= 2 * MAX_NORM and n1 >= 2 * MAX_NORM
    rel = np.linalg.norm((ma - m1).astype(np.float64)) / np.linalg.norm(m1.astype(np.float64))
    print(f'[2 ranks x K=2 vs 1 rank] m rel-L2 {rel:.3e}  norm {na:.6f} vs {n1:.6f}  loss {(la + lb) / 2:.7f} vs {l1:.7f}')
    assert rel <= 4e-5, rel
    assert abs(na - n1) / n1 <= 2e-5
    assert abs((la + lb) / 2 - l1) <= 1e-5 * abs(l1)
