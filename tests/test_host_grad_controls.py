"""CPU tests of the host side of Trainer.apply_grad_args (gradient accumulation + global-norm clipping): the new C ABI symbols resolve,
train() hands train_step_accum K shards per optimizer step at the reference's step / checkpoint cadence, the switch off leaves the
train_step(batch, step) call, micro-step keys, and the CLI flag."""
import ctypes as C
import json

import pytest
import torch


def _mock_trainer(tmp_path, steps=5, every=2, **kw):
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(dim=16, rngs=0, channels=1, device='cpu')
    gd = GaussianDiffusion(unet, image_size=8, num_frames=2, channels=1, timesteps=10)
    return Trainer(gd, str(tmp_path), dataset_path='synthetic:8', train_batch_size=2, train_num_steps=steps,
                   checkpoint_every_steps=every, results_folder=str(tmp_path / 'res'), **kw)


def test_new_symbols_resolve():
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import ops, train_step
    for name in ('vdx_grad_accumulate', 'vdx_grad_sqnorm_scratch_doubles', 'vdx_grad_sqnorm', 'vdx_adam_ema_step_clip'):
        assert getattr(L.lib, name) is not None
    assert train_step.vdx_grad_sqnorm_scratch_doubles() >= 1
    assert callable(ops.grad_accumulate) and callable(ops.grad_sqnorm) and callable(ops.adam_ema_step_clip)
    # argument checks run before anything touches a device: null pointers, n < 1, pointers off the 4-byte grid, max_grad_norm <= 0
    buf = (C.c_float * 8)()
    a = C.addressof(buf)
    assert train_step.vdx_grad_accumulate(0, a, 4, 0) != 0 and b'grad_accumulate' in L.vdx_last_error()
    assert train_step.vdx_grad_accumulate(a, a + 2, 4, 0) != 0
    assert train_step.vdx_grad_accumulate(a, a + 4, 0, 0) != 0
    assert train_step.vdx_grad_sqnorm(a + 1, 4, a, a, 0) != 0 and b'grad_sqnorm' in L.vdx_last_error()
    assert train_step.vdx_adam_ema_step_clip(a, a, a, a, a, 4, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, 1, 0.9, a, 0.0, 0, 0) != 0
    assert b'adam_ema_step_clip' in L.vdx_last_error()


def test_switch_defaults_off_and_allocates_nothing(tmp_path):
    from video_diffusion_nnx_amd.trainer import Trainer
    assert Trainer.apply_grad_args is False and Trainer.track_grad_norm is False
    tr = _mock_trainer(tmp_path, gradient_accumulate_every=3, max_grad_norm=10.0)
    assert tr.accum_steps == 1 and tr.micro_grads is None and tr.last_grad_norm is None
    with pytest.raises(AssertionError):
        tr.train_step_accum([torch.zeros(2, 1, 2, 8, 8)], 0)
    tr.apply_grad_args = True
    assert tr.accum_steps == 3
    tr.gradient_accumulate_every = 0
    assert tr.accum_steps == 1


def test_train_hands_k_shards_per_step_at_the_2_4_5_cadence(tmp_path, monkeypatch):
    tr = _mock_trainer(tmp_path, gradient_accumulate_every=3, max_grad_norm=10.0)
    tr.apply_grad_args = True
    saved, logged, calls = [], [], []

    def fake_accum(batches, step):
        calls.append((len(batches), [tuple(b.shape) for b in batches], step))
        tr.last_grad_norm = torch.tensor([12.5 + step])
        return torch.tensor(1.0)
    monkeypatch.setattr(tr, '_save', lambda step: saved.append(step))
    monkeypatch.setattr(tr, 'train_step_accum', fake_accum)
    monkeypatch.setattr(tr, 'train_step', lambda *a, **k: pytest.fail('train_step called with the switch on'))
    tr.train(log_fn=lambda d: logged.append(d))
    assert [c[2] for c in calls] == [0, 1, 2, 3, 4]                       # step advances once per optimizer step
    assert all(c[0] == 3 and c[1] == [(2, 1, 2, 8, 8)] * 3 for c in calls)
    assert saved == [2, 4, 5] and tr.step == 5
    assert [d['step'] for d in logged] == [0, 1, 2, 3, 4]
    rows = [json.loads(l) for l in open(tr.log_dir / 'scalars_rank0.jsonl')]
    norms = [(r['step'], r['value']) for r in rows if r['tag'] == 'grad_norm/train']
    assert norms == [(s, 12.5 + s) for s in range(5)]


def test_k_shards_are_distinct_batches(tmp_path, monkeypatch):
    tr = _mock_trainer(tmp_path, steps=2, gradient_accumulate_every=2)
    tr.apply_grad_args = True
    seen = []
    monkeypatch.setattr(tr, '_save', lambda step: None)
    monkeypatch.setattr(tr, 'train_step_accum', lambda batches, step: (seen.extend(batches), torch.tensor(1.0))[1])
    tr.train()
    assert len(seen) == 4
    assert not any(torch.equal(seen[i], seen[j]) for i in range(4) for j in range(i))
    rows = [json.loads(l) for l in open(tr.log_dir / 'scalars_rank0.jsonl')]
    assert not [r for r in rows if r['tag'] == 'grad_norm/train']         # no clipping, no norm: nothing logged


def test_switch_off_calls_train_step_as_before(tmp_path, monkeypatch):
    tr = _mock_trainer(tmp_path, gradient_accumulate_every=3, max_grad_norm=10.0)
    calls = []
    monkeypatch.setattr(tr, '_save', lambda step: None)
    monkeypatch.setattr(tr, 'train_step', lambda batch, step: (calls.append((tuple(batch.shape), step)), torch.tensor(1.0))[1])
    monkeypatch.setattr(tr, 'train_step_accum', lambda *a, **k: pytest.fail('train_step_accum called with the switch off'))
    tr.train()
    assert calls == [((2, 1, 2, 8, 8), s) for s in range(5)]
    rows = [json.loads(l) for l in open(tr.log_dir / 'scalars_rank0.jsonl')]
    assert sorted({r['tag'] for r in rows}) == ['loss/train', 'lr/train', 'step_time']


def test_micro_step_keys():
    from video_diffusion_nnx_amd.gaussian_diffusion import split_key
    from video_diffusion_nnx_amd.train_step import micro_step_keys
    for seed, rank, step in ((0, 0, 0), (7, 1, 3), (123, 3, 1000)):
        step_key = split_key(split_key(seed, rank + 1)[-1], step + 1)[-1]            # the plain train step's derivation
        _, t_key, loss_key = split_key(step_key, 3)
        _, noise_key, _ = split_key(loss_key, 3)
        assert micro_step_keys(seed, rank, step, 0) == (t_key, noise_key)
        assert micro_step_keys(seed, rank, step) == (t_key, noise_key)
        keys = [micro_step_keys(seed, rank, step, j) for j in range(4)]
        flat = [k for pair in keys for k in pair]
        assert len(set(flat)) == 8, 'micro-step keys collide'
        micro_key = split_key(step_key, 3 + 2)[-1]                                   # j = 2: child 5 of the step key
        assert keys[2] == (split_key(micro_key, 3)[1], split_key(split_key(micro_key, 3)[2], 3)[1])
        assert set(flat).isdisjoint(micro_step_keys(seed, rank, step + 1, j)[i] for j in range(4) for i in range(2))


def test_train_cli_flag_sets_the_switch(tmp_path, monkeypatch):
    import yaml
    import sample
    import train
    from video_diffusion_nnx_amd import trainer as trainer_mod
    seen = []

    class FakeTrainer:
        apply_grad_args = False

        def __init__(self, **kw):
            seen.append((type(self).apply_grad_args, kw.get('gradient_accumulate_every'), kw.get('max_grad_norm')))

        def train(self):
            pass
    cfg = {'unet': {}, 'diffusion': {}, 'trainer': dict(folder=str(tmp_path), gradient_accumulate_every=2, max_grad_norm=10)}
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    monkeypatch.setattr(sample, 'build_models', lambda cfg, mode: (None, None))
    monkeypatch.setattr(trainer_mod, 'Trainer', FakeTrainer)
    train.main(['--config', str(path)])
    assert seen == [(False, 2, 10)]
    train.main(['--config', str(path), '--apply_grad_args'])
    assert seen[-1] == (True, 2, 10) and FakeTrainer.apply_grad_args is True
    assert trainer_mod.Trainer is FakeTrainer
