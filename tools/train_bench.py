"""Training throughput of the north-star shape (BASELINE.json configs[2]: dim 64, 16f x 64x64, batch 4 per GPU, l2).
    python tools/train_bench.py [--batch 4] [--steps 5] [--mode bf16] [--accum K] [--max-grad-norm X] [--frame-cond-max K]
One process per GPU (launch with torch.distributed.run for N > 1); prints samples/s and ms/step.
--accum K / --max-grad-norm X turn Trainer.apply_grad_args on: a step is then one optimizer step over K micro-batches of --batch
samples each (ms/step is per optimizer step, samples/s counts all K), with the averaged gradient clipped to X.
--frame-cond-max K: frame-conditioned training (Trainer.frame_cond_max), up to K clean context frames per sample."""
import argparse, os, sys, time, tempfile
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4); ap.add_argument('--steps', type=int, default=5); ap.add_argument('--mode', default='bf16')
    ap.add_argument('--dim', type=int, default=64); ap.add_argument('--frames', type=int, default=16); ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--accum', type=int, default=None, help='micro-batches per optimizer step (Trainer.apply_grad_args)')
    ap.add_argument('--max-grad-norm', type=float, default=None, help='global-norm clipping threshold (Trainer.apply_grad_args)')
    ap.add_argument('--frame-cond-max', type=int, default=0, help='frame-conditioned training: up to K context frames (Trainer.frame_cond_max)')
    a = ap.parse_args()
    world = int(os.environ.get('WORLD_SIZE', '1')); local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    from video_diffusion_nnx_amd.gaussian_diffusion import GaussianDiffusion
    from video_diffusion_nnx_amd.trainer import Trainer
    from video_diffusion_nnx_amd.unet3d import Unet3D
    unet = Unet3D(dim=a.dim, rngs=0, channels=1, mode=a.mode)
    gd = GaussianDiffusion(unet, image_size=a.size, num_frames=a.frames, channels=1, timesteps=1000, loss_type='l2')
    tmp = tempfile.mkdtemp()
    grad_args = a.accum is not None or a.max_grad_norm is not None
    K = max(1, a.accum or 1)
    Trainer.apply_grad_args = grad_args
    Trainer.frame_cond_max = a.frame_cond_max
    tr = Trainer(gd, tmp, dataset_path='synthetic:64', train_batch_size=a.batch * world, train_num_steps=10 ** 9, results_folder=tmp,
                 gradient_accumulate_every=K, max_grad_norm=a.max_grad_norm)
    x = torch.rand(a.batch, 1, a.frames, a.size, a.size).to(torch.device('cuda', local))      # resident, as bench.py's train leg
    step = (lambda i: tr.train_step_accum([x] * K, i)) if grad_args else (lambda i: tr.train_step(x, i))
    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss = step(2 + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    if int(os.environ.get('RANK', '0')) == 0:
        extra = f' accum={K} max_grad_norm={a.max_grad_norm} {dt*1e3/K:.2f} ms/micro-batch' if grad_args else ''
        extra += f' frame_cond_max={a.frame_cond_max}' if a.frame_cond_max else ''
        print(f'train: mode={a.mode} world={world} batch/gpu={a.batch} {dt*1e3:.1f} ms/step {a.batch*K*world/dt:.2f} samples/s loss={loss.item():.4f}{extra}',
              flush=True)


if __name__ == '__main__':
    main()
