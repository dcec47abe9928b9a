"""MovingMNIST .npy loader mirroring the reference's datasets.py:11-64 as it BEHAVES (no resize, no /255: values stay
raw floats, (F,B,H,W) -> per item (1, frames, H, W) with pad/truncate), plus a synthetic source for benchmarks.
NumPy only (torchvision is not needed: the reference builds a transform pipeline but never applies it)."""
from __future__ import annotations

import numpy as np
import torch
import torch.utils.data as data

from functools import partial

from .utils import cast_num_frames, identity


class MovingMNIST(data.Dataset):
    def __init__(self, file_path, image_size, channels=1, num_frames=20, horizontal_flip=False, force_num_frames=True):
        super().__init__()
        self.file_path, self.image_size, self.channels = file_path, image_size, channels
        self.channnels = channels                                     # the reference's attribute name (datasets.py:38)
        arr = np.load(file_path)                                      # (f, b, h, w)
        arr = np.transpose(arr, (1, 0, 2, 3))[:, None, ...]           # (b, 1, f, h, w)
        self.arrays = arr.astype(np.float32)
        # datasets.py:47-48: a functools.partial (the reference's tests read .keywords['frames']) or the identity
        self.cast_num_frames_fn = partial(cast_num_frames, frames=num_frames) if force_num_frames else identity
        self.cast = self.cast_num_frames_fn

    def __len__(self):
        return self.arrays.shape[0]

    def __getitem__(self, index):
        return self.cast(self.arrays[index])


class SyntheticVideo(data.Dataset):
    """`dataset_path: synthetic:N` -> N seeded uniform [0,1) videos of shape (channels, frames, size, size)."""

    def __init__(self, n, channels, num_frames, image_size, seed=0):
        self.n, self.shape, self.seed = int(n), (channels, num_frames, image_size, image_size), seed

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 1000003 + int(index))
        return torch.rand(self.shape, generator=g).numpy()


def load_cond_file(path, n_items: int, cond_dim: int) -> np.ndarray:
    """Trainer.cond_path: the float32 [N, cond_dim] array of a .npy file; row i is the condition of video i of a dataset of n_items
    videos.  Another N or cond_dim raises ValueError."""
    arr = np.load(path)
    if arr.ndim != 2 or arr.shape[0] != int(n_items) or arr.shape[1] != int(cond_dim):
        raise ValueError(f'{path}: expected a [{int(n_items)}, {int(cond_dim)}] array (one row of cond_dim floats per video), '
                         f'got shape {tuple(arr.shape)}')
    return np.ascontiguousarray(arr, dtype=np.float32)


class CondPairs(data.Dataset):
    """(video, cond_row) pairs: item i of `videos` with row i of `conds` [N, cond_dim], so a shuffling loader keeps them together."""

    def __init__(self, videos, conds):
        if len(videos) != len(conds):
            raise ValueError(f'{len(conds)} condition rows for {len(videos)} videos')
        self.videos, self.conds = videos, conds

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, index):
        return self.videos[index], self.conds[index]


class DevicePrefetcher:
    """Host -> device staging of the training batches (reference trainer.py:546-547 hands each host batch to a synchronous
    `device_put` inside the step).  One batch ahead: the NEXT batch's shard is copied into a pinned host buffer and
    sent to the GPU on a side stream while the current step runs, so `Trainer.train()` never waits on PCIe.  `next()` returns a
    device tensor whose copy the CURRENT stream has been made to wait for.  Without a GPU (CPU tests) it passes batches through.

    `select(batch) -> shard` picks this rank's slice (P('data', None), trainer.py:309).  A tuple or list batch (the (video, cond) pairs
    of CondPairs) is staged element by element -- each pinned, on the side stream, sharded by `select` -- and comes back as a tuple."""

    def __init__(self, iterator, device, select=None):
        self.it, self.device, self.select = iterator, torch.device(device), (select or (lambda b: b))
        self.on_gpu = self.device.type == 'cuda' and torch.cuda.is_available()
        self.stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        self._pinned = [None, None]                                   # two pinned staging buffers (lists of them for tuple batches), used alternately
        self._copied = [None, None]                                   # event behind the last H2D copy OUT of each buffer
        self._k = 0
        self._next = None
        self._stage()

    def _stage(self):
        try:
            item = next(self.it)
        except StopIteration:
            self._next = None
            return
        many = isinstance(item, (tuple, list))
        hosts = [self.select(torch.as_tensor(np.asarray(e))).to(torch.float32) for e in (item if many else (item,))]
        if not self.on_gpu:
            hosts = [h.contiguous() for h in hosts]
            self._next = (tuple(hosts) if many else hosts[0], None)
            return
        bufs = self._pinned[self._k]                                  # a tensor for a single-tensor batch, a list of them for a tuple batch
        bufs = [bufs] if torch.is_tensor(bufs) else bufs
        if bufs is None or [b.shape for b in bufs] != [h.shape for h in hosts]:
            bufs = [torch.empty(h.shape, dtype=torch.float32).pin_memory() for h in hosts]
        self._pinned[self._k] = bufs if many else bufs[0]
        k = self._k
        self._k ^= 1
        if self._copied[k] is not None:
            self._copied[k].synchronize()                             # the DMA that read these buffers two batches ago has finished (almost always already true)
        for buf, host in zip(bufs, hosts):
            buf.copy_(host)
        with torch.cuda.stream(self.stream):
            devs = [buf.to(self.device, non_blocking=True) for buf in bufs]
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._copied[k] = ev
        self._next = (tuple(devs) if many else devs[0], ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        dev, ev = self._next
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)    # device-side wait only: the host does not block
            for d in (dev if isinstance(dev, tuple) else (dev,)):
                d.record_stream(torch.cuda.current_stream(self.device))
        self._stage()                                                 # the following batch goes out while this one is consumed
        return dev
